"""GPU: slot heads -- sir_ce_loss_slots, sir_classify_slots and sir_eval_accumulate_slots (include/sir_hip.h "slot heads").

1. bit identity, per slot, with sir_ce_loss_soft / sir_classify / sir_eval_accumulate on contiguous copies of the segment;
2. the joint quantities against the float64 reference (tests/slots_ref.py);
3. the row kinds (-100, bad label, non-finite segment, ties, k above a width, zero weight, width-1 slot);
4. refused calls write nothing;
5. the Python surface (sir_amd/slots.py, train(), evaluate(), results dictionaries).

The inputs are ``slots_ref.case``'s; tests/test_slots_host.py asserts, for every row, that no ranking or bin of theirs hangs on
a rounding."""
import ctypes as C
import json
import os
import types

import numpy as np
import pandas as pd
import pytest
import torch
import torch.nn.functional as F

import eval_ref
import slots_ref
from oracle import model_ref
from sir_amd import _native, metrics, ops, slots, synth, train_ops
from sir_amd.featurizer import get_featurizer
from sir_amd.models.models import CNNAudioGRU
from sir_amd.optim import FusedAdam

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
M = slots_ref.N_BINS
SENT = -7.0


def _id(sizes):
    return "x".join(map(str, sizes)) if len(set(sizes)) > 1 else f"{sizes[0]}x{len(sizes)}"


layouts = pytest.mark.parametrize("sizes", slots_ref.LAYOUTS, ids=_id)
batches = pytest.mark.parametrize("batch", slots_ref.BATCHES)


def _dev(t):
    return None if t is None else t.to(DEV)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _sizes(sizes):
    return (C.c_int32 * len(sizes))(*sizes)


def _stream():
    return _native.current_stream_ptr()


# ---- raw calls: every output starts as a sentinel -----------------------------------------------------------------------------
def _raw_ce(lg, ya, yb, lam, eps, sizes, weights=None, grad_scale=1.0, n_slots=None, num_classes=None):
    g = len(sizes)
    loss = torch.full((1,), SENT, device=DEV)
    slot_loss = torch.full((max(g, 1),), SENT, device=DEV)
    d = torch.full_like(lg, SENT)
    w = (C.c_float * len(weights))(*weights) if weights is not None else None
    rc = _native.lib().sir_ce_loss_slots(get_featurizer().handle, lg.data_ptr(), ya.data_ptr(), _ptr(yb), _ptr(lam), eps, _sizes(sizes), w,
                                         g if n_slots is None else n_slots, lg.shape[0], lg.shape[1] if num_classes is None else num_classes,
                                         loss.data_ptr(), slot_loss.data_ptr(), d.data_ptr(), grad_scale, _stream())
    return rc, loss, slot_loss, d


def _single_ce(seg, ya, yb, lam, eps, grad_scale):
    loss = torch.full((1,), SENT, device=DEV)
    d = torch.full_like(seg, SENT)
    rc = _native.lib().sir_ce_loss_soft(get_featurizer().handle, seg.data_ptr(), ya.data_ptr(), _ptr(yb), _ptr(lam), eps, seg.shape[0],
                                        seg.shape[1], loss.data_ptr(), d.data_ptr(), grad_scale, _stream())
    assert rc == 0
    return loss, d


def _raw_classify(lg, sizes, k, beta=None, n_slots=None, num_classes=None):
    b, g = lg.shape[0], len(sizes)
    probs = torch.full_like(lg, SENT)
    idx = torch.full((b, max(g, 1), max(k, 1)), -7, dtype=torch.int32, device=DEV)
    top = torch.full((b, max(g, 1), max(k, 1)), SENT, device=DEV)
    joint = torch.full((b,), SENT, device=DEV)
    rc = _native.lib().sir_classify_slots(get_featurizer().handle, lg.data_ptr(), b, lg.shape[1] if num_classes is None else num_classes,
                                          _sizes(sizes), g if n_slots is None else n_slots, _ptr(beta), k, probs.data_ptr(), idx.data_ptr(),
                                          top.data_ptr(), joint.data_ptr(), _stream())
    return rc, probs, idx, top, joint


def _raw_eval(lg, y, sizes, state, beta=None, n_bins=M, state_bytes=None, n_slots=None, num_classes=None):
    return _native.lib().sir_eval_accumulate_slots(get_featurizer().handle, lg.data_ptr(), y.data_ptr(), lg.shape[0],
                                                   lg.shape[1] if num_classes is None else num_classes, _sizes(sizes),
                                                   len(sizes) if n_slots is None else n_slots, _ptr(beta), n_bins, state.data_ptr(),
                                                   state.numel() * 8 if state_bytes is None else state_bytes, _stream())


def _new_state(sizes, n_bins=M):
    return torch.zeros(slots.state_words(sizes, n_bins), dtype=torch.int64, device=DEV)


def _beta_dev(sizes):
    return torch.tensor(slots_ref.betas_of(sizes), dtype=torch.float32, device=DEV)


def _segs(lg, sizes):
    return [lg[:, a:b].contiguous() for a, b in slots_ref.segments(sizes)]


def _col(y, g):
    return None if y is None else y[:, g].contiguous()


# ---- 1. bit identity ----------------------------------------------------------------------------------------------------------
@layouts
@batches
def test_loss_is_bit_identical_per_slot_to_ce_loss_soft(sizes, batch):
    for second, eps in ((False, 0.0), (True, 0.1), (False, 0.1)):
        logits, ya, yb, lam = slots_ref.case(sizes, batch, second)
        lg, ya, yb, lam = _dev(logits), _dev(ya), _dev(yb), _dev(lam)
        w = slots_ref.weights_of(sizes)
        rc, loss, slot_loss, d = _raw_ce(lg, ya, yb, lam, eps, sizes, w, grad_scale=3.0)
        assert rc == 0
        want_total = np.float32(0.0)
        for g, (seg, (a, b)) in enumerate(zip(_segs(lg, sizes), slots_ref.segments(sizes))):
            gs = float(np.float32(3.0) * np.float32(w[g]))                                 # the fp32 product, formed on the host
            want_loss, want_d = _single_ce(seg, _col(ya, g), _col(yb, g), lam, eps, gs)
            assert torch.equal(slot_loss[g:g + 1], want_loss), (g, second, eps)
            assert torch.equal(d[:, a:b], want_d), (g, second, eps)
            want_total = np.float32(want_total + np.float32(np.float32(w[g]) * np.float32(want_loss.item())))
        assert loss.item() == want_total                                                   # fp32 products added in slot order
        if len(sizes) == 1:                                                                # one slot: the existing call in every output
            for weights in (None, [1.0]):
                rc, loss1, slot1, d1 = _raw_ce(lg, ya, yb, lam, eps, sizes, weights, grad_scale=3.0)
                want_loss, want_d = _single_ce(lg, _col(ya, 0), _col(yb, 0), lam, eps, 3.0)
                assert rc == 0 and torch.equal(loss1, want_loss) and torch.equal(slot1, want_loss) and torch.equal(d1, want_d)
    ops.check_status()


@layouts
@batches
def test_classification_is_bit_identical_per_slot_to_classify(sizes, batch):
    lg = _dev(slots_ref.case(sizes, batch)[0])
    lib, h = _native.lib(), get_featurizer().handle
    for k in (1, 3, 8):
        for beta in (None, _beta_dev(sizes)):
            rc, probs, idx, top, joint = _raw_classify(lg, sizes, k, beta)
            assert rc == 0
            want_joint = torch.ones(batch, device=DEV)
            for g, (seg, (a, b)) in enumerate(zip(_segs(lg, sizes), slots_ref.segments(sizes))):
                kk = min(k, b - a)
                p1 = torch.empty_like(seg)
                i1 = torch.empty((batch, kk), dtype=torch.int32, device=DEV)
                t1 = torch.empty((batch, kk), device=DEV)
                assert lib.sir_classify(h, seg.data_ptr(), batch, b - a, None if beta is None else beta[g:].data_ptr(), kk, p1.data_ptr(),
                                        i1.data_ptr(), t1.data_ptr(), _stream()) == 0
                assert torch.equal(probs[:, a:b], p1) and torch.equal(idx[:, g, :kk], i1) and torch.equal(top[:, g, :kk], t1), (g, k)
                assert (idx[:, g, kk:] == -1).all() and (top[:, g, kk:] == 0).all()
                want_joint = want_joint * t1[:, 0]                                         # fp32, slot order
            assert torch.equal(joint, want_joint)


@layouts
@batches
def test_slot_states_are_bit_identical_to_eval_accumulate(sizes, batch):
    logits, ya, _, _ = slots_ref.case(sizes, batch)
    lg, y = _dev(logits), _dev(ya)
    lib, h = _native.lib(), get_featurizer().handle
    for beta in (None, _beta_dev(sizes)):
        state = _new_state(sizes)
        for _ in range(2):                                                                 # calls into one state add up
            assert _raw_eval(lg, y, sizes, state, beta) == 0
        o = 0
        for g, seg in enumerate(_segs(lg, sizes)):
            c = sizes[g]
            single = torch.zeros(metrics.state_words(c, M), dtype=torch.int64, device=DEV)
            for _ in range(2):
                assert lib.sir_eval_accumulate(h, seg.data_ptr(), _col(y, g).data_ptr(), batch, c, None if beta is None else beta[g:].data_ptr(),
                                               M, single.data_ptr(), single.numel() * 8, _stream()) == 0
            n = metrics.field_words(c, M)
            assert torch.equal(state[o: o + n], single[:n]), g                             # integers and the doubles' bit patterns
            o += metrics.state_words(c, M)
    ops.check_status()


# ---- 2. float64 ---------------------------------------------------------------------------------------------------------------
@layouts
@batches
def test_loss_gradient_and_joint_quantities_vs_float64(sizes, batch):
    """loss within 1e-5 absolute (the bound of every loss comparison, tests/test_recipe_gpu.py); dlogits per element within
    that file's (C_g + 8 + R) * 2^-24 / n_valid_g, scaled by w_g (the weights are powers of two and their sums of two: the
    product grad_scale * w_g is exact at grad_scale 1); joint_prob within 4e-6 * n_slots (tests/test_eval_gpu.py's bound on one
    probability, once per factor); the joint nll_sum / bin_conf_sum within rel 1e-6 (same file); the joint integers exact."""
    logits, ya, yb, lam = slots_ref.case(sizes, batch, second=True)
    w = slots_ref.weights_of(sizes)
    lg = logits.to(DEV).requires_grad_(True)
    loss, slot_losses = slots.slot_cross_entropy(lg, _dev(ya), sizes, w, _dev(yb), _dev(lam), 0.1, return_slot_losses=True)
    loss.backward()
    ref_loss, ref_slots, ref_d = slots_ref.soft_ce_slots(logits, ya, sizes, w, yb, lam, 0.1)
    err = abs(loss.item() - ref_loss.item())
    derr = (lg.grad.cpu().double() - ref_d).abs()
    worst = 0.0
    for g, (a, b) in enumerate(slots_ref.segments(sizes)):
        seg = logits[:, a:b]
        spread = (seg.max(dim=1).values - seg.min(dim=1).values).double()[:, None]
        bound = (sizes[g] + 8 + spread) * U / int((ya[:, g] != -100).sum()) * w[g]
        worst = max(worst, (derr[:, a:b] / bound).max().item())
        assert (derr[:, a:b] <= bound).all(), g
        assert (lg.grad[:, a:b][_dev(ya[:, g] == -100)] == 0).all()
    assert (slot_losses.cpu().double() - ref_slots).abs().max().item() <= 1e-5
    for betas in (None, slots_ref.betas_of(sizes)):
        idx, top, joint = slots.classify(lg.detach(), sizes, k=1, inv_temperature=betas)
        _, ref_idx, _, ref_joint = slots_ref.classify_slots(logits, sizes, 1, betas)
        assert np.array_equal(idx.cpu().numpy(), ref_idx)
        jerr = np.abs(joint.cpu().numpy().astype(np.float64) - ref_joint).max()
        acc = slots.SlotEvalAccumulator(sizes, n_bins=M, inv_temperature=betas).update(lg.detach(), _dev(ya))
        got = acc.state_arrays()["joint"]
        want = slots_ref.eval_accumulate_slots(slots_ref.empty_state(sizes, M), logits, ya, sizes, M, betas)["joint"]
        for f in ("n", "exact_match", "n_excluded"):
            assert got[f] == want[f], f
        for f in ("slots_correct", "bin_count", "bin_correct"):
            assert np.array_equal(got[f], want[f]), f
        rel_nll = abs(got["nll_sum"] - want["nll_sum"]) / max(abs(want["nll_sum"]), 1e-300)
        print(f"slots {sizes} B={batch} betas={'set' if betas else None}: |loss - ref| {err:.2e}, dlogits err / bound {worst:.3f}, "
              f"joint_prob err {jerr:.2e} (bound {4e-6 * len(sizes):.1e}), joint nll rel {rel_nll:.2e}")
        assert jerr <= 4e-6 * len(sizes)
        assert got["nll_sum"] == pytest.approx(want["nll_sum"], rel=1e-6, abs=1e-12)
        assert np.allclose(got["bin_conf_sum"], want["bin_conf_sum"], rtol=1e-6, atol=0)
    assert err <= 1e-5
    ops.check_status()


# ---- 3. row kinds -------------------------------------------------------------------------------------------------------------
FSC = (6, 14, 4)


def _eval_arrays(lg, y, sizes, beta=None):
    state = _new_state(sizes)
    assert _raw_eval(lg, y, sizes, state, beta) == 0
    return slots.unpack_state(state.cpu().numpy(), sizes, M), state


def _same_slot(a, b):
    return all(np.array_equal(a[f], b[f]) for f in metrics._INT_FIELDS + metrics._FLOAT_FIELDS)


def test_ignore_label_in_one_slot_only():
    logits, ya, _, _ = slots_ref.case(FSC, 17)
    lg = _dev(logits)
    _, loss0, sl0, d0 = _raw_ce(lg, _dev(ya), None, None, 0.0, FSC)
    st0, _ = _eval_arrays(lg, _dev(ya), FSC)
    yb = ya.clone()
    yb[5, 1] = -100
    rc, loss1, sl1, d1 = _raw_ce(lg, _dev(yb), None, None, 0.0, FSC)
    st1, _ = _eval_arrays(lg, _dev(yb), FSC)
    assert rc == 0 and torch.equal(sl1[[0, 2]], sl0[[0, 2]]) and not torch.equal(sl1[1], sl0[1])
    assert torch.equal(d1[:, :6], d0[:, :6]) and torch.equal(d1[:, 20:], d0[:, 20:]) and (d1[5, 6:20] == 0).all()
    # the slot's divisor moved from 17 to 16: every other row's gradient in that segment grows by 17 / 16
    rows = [i for i in range(17) if i != 5]
    assert torch.allclose(d1[rows, 6:20], d0[rows, 6:20] * (17.0 / 16.0), rtol=1e-6, atol=0)
    want = slots_ref.soft_ce_slots(logits, yb, FSC)[1][1].item()
    assert abs(sl1[1].item() - want) <= 1e-5
    assert st1["slots"][1]["n"] == st0["slots"][1]["n"] - 1 == 16 and st1["slots"][1]["n_ignored"] == st0["slots"][1]["n_ignored"] + 1 == 1
    assert _same_slot(st1["slots"][0], st0["slots"][0]) and _same_slot(st1["slots"][2], st0["slots"][2])
    assert st1["joint"]["n_excluded"] == st0["joint"]["n_excluded"] + 1 == 3 and st1["joint"]["n"] == 14
    ops.check_status()


def test_out_of_range_label_in_one_slot():
    logits, ya, yb, lam = slots_ref.case(FSC, 17, second=True)
    lg = _dev(logits)
    _, _, sl0, _ = _raw_ce(lg, _dev(ya), None, None, 0.0, FSC)
    st0, _ = _eval_arrays(lg, _dev(ya), FSC)
    ops.check_status()
    for bad in (14, -1):
        y = ya.clone()
        y[4, 1] = bad
        rc, loss, sl, d = _raw_ce(lg, _dev(y), None, None, 0.0, FSC)
        assert rc == 0 and torch.isnan(loss).item() and torch.isnan(sl[1]).item() and torch.equal(sl[[0, 2]], sl0[[0, 2]])
        with pytest.raises(_native.SirError):
            ops.check_status()
        ops.check_status()                                                                 # (reported once, then cleared)
        st, _ = _eval_arrays(lg, _dev(y), FSC)
        with pytest.raises(_native.SirError):
            ops.check_status()
        s1, c1 = st["slots"][1], st0["slots"][1]
        assert s1["n"] == c1["n"] - 1 and s1["n_ignored"] == c1["n_ignored"] and s1["n_nonfinite"] == c1["n_nonfinite"]
        assert s1["confusion"].sum() == c1["confusion"].sum() - 1 and s1["bin_count"].sum() == c1["bin_count"].sum() - 1
        assert _same_slot(st["slots"][0], st0["slots"][0]) and _same_slot(st["slots"][2], st0["slots"][2])
        assert st["joint"]["n_excluded"] == st0["joint"]["n_excluded"] + 1 and st["joint"]["n"] == st0["joint"]["n"] - 1
    # a bad SECOND label is flagged the same way
    y2 = yb.clone()
    y2[4, 2] = 4
    rc, loss, sl, _ = _raw_ce(lg, _dev(ya), _dev(y2), _dev(lam), 0.1, FSC)
    assert rc == 0 and torch.isnan(loss).item() and torch.isnan(sl[2]).item() and torch.isfinite(sl[:2]).all()
    with pytest.raises(_native.SirError):
        ops.check_status()
    ops.check_status()


def test_non_finite_value_in_one_segment_only():
    logits, ya, _, _ = slots_ref.case(FSC, 17)
    clean = _raw_classify(_dev(logits), FSC, 3)
    st0, _ = _eval_arrays(_dev(logits), _dev(ya), FSC)
    x = logits.clone()
    x[3, 7] = float("nan")                                                               # slot 1
    x[9, 23] = float("inf")                                                              # slot 2, last column
    x[12, 0] = -float("inf")                                                             # slot 0, first column
    rc, probs, idx, top, joint = _raw_classify(_dev(x), FSC, 3)
    assert rc == 0
    hit = {(3, 1), (9, 2), (12, 0)}
    for b in range(17):
        for g, (a, e) in enumerate(slots_ref.segments(FSC)):
            if (b, g) in hit:
                assert (idx[b, g] == -1).all() and torch.isnan(top[b, g]).all() and torch.isnan(probs[b, a:e]).all()
            else:
                assert torch.equal(idx[b, g], clean[2][b, g]) and torch.equal(top[b, g], clean[3][b, g]) and torch.equal(probs[b, a:e], clean[1][b, a:e])
    bad_rows = [3, 9, 12]
    good = [b for b in range(17) if b not in bad_rows]
    assert torch.isnan(joint[bad_rows]).all() and torch.equal(joint[good], clean[4][good])
    st, _ = _eval_arrays(_dev(x), _dev(ya), FSC)
    want = slots_ref.eval_accumulate_slots(slots_ref.empty_state(FSC, M), x, ya, FSC, M)
    for g in range(3):
        assert st["slots"][g]["n_nonfinite"] == 1 == want["slots"][g]["n_nonfinite"] and st["slots"][g]["n"] == st0["slots"][g]["n"] - 1
        assert np.array_equal(st["slots"][g]["confusion"], want["slots"][g]["confusion"])
    assert st["joint"]["n_excluded"] == want["joint"]["n_excluded"] == 5 and st["joint"]["n"] == want["joint"]["n"] == 12
    ops.check_status()


def test_ties_inside_a_slot():
    sizes = (6, 14, 4)
    x = torch.linspace(-3.0, -1.0, 24).repeat(4, 1)
    x[0, [9, 17]] = 5.0                                       # slot 1: two equal maxima (local 3 and 11)
    x[1, 6:20] = 0.25                                         # slot 1: all equal
    x[2, [20, 23]] = 1.0                                      # slot 2: first and last column
    x[3, 1], x[3, 0] = 0.0, -0.0                              # slot 0: +0 and -0 compare equal, the lower index first
    y = torch.tensor([[5, 11, 3], [5, 0, 3], [5, 13, 3], [1, 13, 3]])
    rc, _, idx, top, joint = _raw_classify(_dev(x), sizes, 3)
    want = slots_ref.classify_slots(x, sizes, 3)
    assert rc == 0 and np.array_equal(idx.cpu().numpy(), want[1])
    got = idx.cpu().numpy()
    assert got[0, 1].tolist() == [3, 11, 13] and got[1, 1].tolist() == [0, 1, 2] and got[2, 2].tolist() == [0, 3, 2] and got[3, 0].tolist()[:2] == [0, 1]
    assert top[1, 1, 0] == top[1, 1, 1] == top[1, 1, 2] and abs(top[1, 1, 0].item() - 1 / 14) < 1e-7
    assert np.abs(joint.cpu().numpy() - want[3]).max() <= 4e-6 * 3
    st, _ = _eval_arrays(_dev(x), _dev(y), sizes)
    ref = slots_ref.eval_accumulate_slots(slots_ref.empty_state(sizes, M), x, y, sizes, M)
    for g in range(3):
        assert np.array_equal(st["slots"][g]["confusion"], ref["slots"][g]["confusion"])
        assert np.array_equal(st["slots"][g]["topk_correct"], ref["slots"][g]["topk_correct"])
    assert st["slots"][1]["confusion"][11, 3] == 1                                       # the tie's second index is a miss
    assert np.array_equal(st["joint"]["slots_correct"], ref["joint"]["slots_correct"]) and st["joint"]["exact_match"] == ref["joint"]["exact_match"]


@pytest.mark.parametrize("sizes", [(6, 14, 4), (1, 63), (2, 2, 2, 2, 2, 2, 2, 50)], ids=_id)
def test_k_above_a_slots_width_is_padded(sizes):
    logits = slots_ref.case(sizes, 17)[0]
    rc, _, idx, top, _ = _raw_classify(_dev(logits), sizes, 8)
    _, want_i, want_t, _ = slots_ref.classify_slots(logits, sizes, 8)
    assert rc == 0 and np.array_equal(idx.cpu().numpy(), want_i)
    assert np.abs(top.cpu().numpy().astype(np.float64) - want_t).max() <= 64 * U          # tests/test_eval_gpu.py PROB_TOL
    for g, c in enumerate(sizes):
        assert (idx[:, g, min(c, 8):] == -1).all() and (top[:, g, min(c, 8):] == 0).all() and (idx[:, g, :min(c, 8)] >= 0).all()


def test_zero_weight_gives_an_exactly_zero_segment():
    logits, ya, yb, lam = slots_ref.case(FSC, 17, second=True)
    for second, eps in ((False, 0.0), (True, 0.1)):
        rc, loss, sl, d = _raw_ce(_dev(logits), _dev(ya), _dev(yb) if second else None, _dev(lam) if second else None, eps, FSC,
                                  [1.0, 0.0, 2.0], grad_scale=3.0)
        assert rc == 0 and (d[:, 6:20] == 0).all() and (d[:, :6] != 0).any() and (d[:, 20:] != 0).any()
        assert torch.isfinite(sl).all() and sl[1].item() > 0                             # the slot's own loss is still reported
        assert loss.item() == np.float32(np.float32(sl[0].item()) + np.float32(2.0) * np.float32(sl[2].item()))


@pytest.mark.parametrize("sizes", [(1, 63), (1,) * 8, (1,)], ids=_id)
def test_width_one_slot_has_probability_one_and_no_loss(sizes):
    logits, ya, _, _ = slots_ref.case(sizes, 17)
    rc, loss, sl, d = _raw_ce(_dev(logits), _dev(ya), None, None, 0.0, sizes)
    rc2, probs, idx, top, joint = _raw_classify(_dev(logits), sizes, 1)
    assert rc == 0 and rc2 == 0
    for g, (a, b) in enumerate(slots_ref.segments(sizes)):
        if b - a == 1:
            assert sl[g].item() == 0.0 and (d[:, a] == 0).all() and (probs[:, a] == 1.0).all() and (idx[:, g, 0] == 0).all()
    if max(sizes) == 1:
        assert loss.item() == 0.0 and (joint == 1.0).all()
        st, _ = _eval_arrays(_dev(logits), _dev(ya), sizes)
        n = 17 - int((ya == -100).any(dim=1).sum())
        assert st["joint"]["n"] == st["joint"]["exact_match"] == st["joint"]["bin_count"][M - 1] == n and st["joint"]["nll_sum"] == 0.0
    ops.check_status()


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing():
    logits, ya, _, _ = slots_ref.case(FSC, 17)
    lg, y = _dev(logits), _dev(ya)
    EINVAL, ENOMEM = _native.SIR_EINVAL, _native.SIR_ENOMEM

    def untouched(*ts):
        return all(bool((t == (SENT if t.is_floating_point() else -7)).all()) for t in ts)

    bad_layouts = [dict(sizes=(6, 14, 5)), dict(sizes=(6, 14, 3)), dict(sizes=(6, 14, 4), n_slots=0), dict(sizes=(3,) * 9, num_classes=27),
                   dict(sizes=(6, 0, 18)), dict(sizes=(6, -1, 19)), dict(sizes=(6, 14, 4), num_classes=65)]
    for kw in bad_layouts:
        rc, *outs = _raw_ce(lg, y, None, None, 0.0, **kw)
        assert rc == EINVAL and untouched(*outs), kw
        rc, *outs = _raw_classify(lg, k=3, **kw)
        assert rc == EINVAL and untouched(*outs), kw
        state = torch.full((slots.state_words(FSC, M),), -7, dtype=torch.int64, device=DEV)
        assert _raw_eval(lg, y, state=state, **kw) == EINVAL and untouched(state), kw
    for k in (0, 9, -1):
        rc, *outs = _raw_classify(lg, FSC, k)
        assert rc == EINVAL and untouched(*outs), k
    for w in ([1.0, float("nan"), 1.0], [1.0, -0.5, 1.0], [float("inf"), 1.0, 1.0]):
        rc, *outs = _raw_ce(lg, y, None, None, 0.0, FSC, w)
        assert rc == EINVAL and untouched(*outs), w
    for eps in (1.0, -0.1, float("nan")):
        rc, *outs = _raw_ce(lg, y, None, None, eps, FSC)
        assert rc == EINVAL and untouched(*outs), eps
    state = torch.full((slots.state_words(FSC, M),), -7, dtype=torch.int64, device=DEV)
    assert _raw_eval(lg, y, FSC, state, state_bytes=state.numel() * 8 - 8) == ENOMEM and untouched(state)
    assert _raw_eval(lg, y, FSC, state, n_bins=0) == EINVAL and _raw_eval(lg, y, FSC, state, n_bins=65) == EINVAL and untouched(state)
    lib, h = _native.lib(), get_featurizer().handle
    assert lib.sir_eval_accumulate_slots(h, lg.data_ptr(), y.data_ptr(), 17, 24, _sizes(FSC), 3, None, M, state.data_ptr() + 4,
                                         state.numel() * 8, _stream()) == EINVAL and untouched(state)
    assert lib.sir_ce_loss_slots(h, lg.data_ptr(), None, None, None, 0.0, _sizes(FSC), None, 3, 17, 24, state.data_ptr(), None, None, 1.0,
                                 _stream()) == EINVAL and untouched(state)
    torch.cuda.synchronize()
    ops.check_status()


# ---- 5. through the surface ---------------------------------------------------------------------------------------------------
def _model(ncls, sd=None):
    m = CNNAudioGRU(ncls)
    m.load_state_dict(sd if sd is not None else synth.synth_state_dict(ncls, seed=0))
    m = m.to(DEV).train()
    m.gru.dropout = 0.0
    return m


def _slot_labels(n, sizes, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randint(0, c, (n,), generator=g) for c in sizes], dim=1)


def test_slot_loss_under_mixup_and_the_adversary_matches_inline_steps():
    """train_epoch with a SlotLoss, mixup and the adversary: the same bits as the steps written out by hand -- [B, G] labels are
    permuted with their rows, both label sets and the per-row lam reach sir_ce_loss_slots, the adversary crafts against it."""
    from sir_amd.feature_store import FeatureStore
    from sir_amd.scripts.train import train_epoch
    n, bsz, t = 14, 6, 16                                                                 # (the last batch is ragged: 2 items)
    feats = synth.synth_features(n, t, seed=9).to(DEV)
    labels = _slot_labels(n, FSC, 10).to(DEV)
    store = FeatureStore.from_tensors(feats, [t] * n, labels)
    kw = dict(shuffle=True, seed=3, epoch=1)
    crit = slots.SlotLoss(FSC, [1.0, 0.5, 2.0], label_smoothing=0.1)

    ma = _model(24)
    oa = FusedAdam(ma.parameters(), lr=1e-3, weight_decay=1e-4)
    mx, adv = train_ops.Mixup(0.2, seed=5), train_ops.Adversary(0.05, steps=1, seed=7)
    ref_losses = []
    for mel, label in store.epoch_batches(bsz, **kw):
        assert label.shape == (mel.shape[0], 3)
        oa.zero_grad(set_to_none=True)
        mixed, label_b, lam = mx(mel, label)
        mixed = adv(ma, mixed, lambda out: crit(out, label, label_b, lam))
        loss = crit(ma(mixed), label, label_b, lam)
        loss.backward()
        oa.step()
        ref_losses.append(loss.detach())
    assert crit.last_slot_losses.shape == (3,) and torch.isfinite(crit.last_slot_losses).all()
    ref_mean = torch.stack(ref_losses).mean().item()

    mb = _model(24)
    ob = FusedAdam(mb.parameters(), lr=1e-3, weight_decay=1e-4)
    train_ops.set_adversary(mb, train_ops.Adversary(0.05, steps=1, seed=7))
    mean = train_epoch(mb, store.epoch_batches(bsz, **kw), ob, slots.SlotLoss(FSC, [1.0, 0.5, 2.0], label_smoothing=0.1), DEV,
                       mixup=train_ops.Mixup(0.2, seed=5))
    torch.cuda.synchronize()
    assert mean == ref_mean and np.isfinite(mean)
    for (name, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        assert torch.equal(pa, pb), name
    # the mixed loss is the float64 reference's, on the logits the model produced
    mel, label = next(iter(store.epoch_batches(bsz, **kw)))
    perm, lam = train_ops.Mixup(0.2, seed=5).draw(bsz)
    with torch.no_grad():
        out = mb(train_ops.mix_features(mel, perm.to(DEV), lam.to(DEV)))
    got = crit(out, label, label[perm.to(DEV)], lam.to(DEV)).item()
    want = slots_ref.soft_ce_slots(out.cpu(), label.cpu(), FSC, [1.0, 0.5, 2.0], label.cpu()[perm], lam, 0.1)[0].item()
    assert abs(got - want) <= 1e-5
    ops.check_status()


def test_three_optimiser_steps_match_torch_float64():
    """Batch 8 of 16 frames, layout (6, 14, 4), dropout off, lr / weight decay of the recipe tests: three steps of
    SlotLoss + FusedAdam against oracle.model_ref.TrainRef in float64 with sum_g w_g F.cross_entropy(segment g) and
    torch.optim.Adam.  Per-step loss bound 1e-4, as tests/test_recipe_gpu.py::test_three_recipe_steps_match_torch_float64."""
    import cases
    w, eps = [1.0, 0.5, 2.0], 0.1
    sd = synth.synth_state_dict(24, seed=0)
    x = synth.synth_features(8, 16, seed=9)
    y = _slot_labels(8, FSC, 11)
    y[3, 2] = -100
    ref = model_ref.TrainRef(sd, 24).double().train()
    ref.load_state_dict({n: (v.double() if v.is_floating_point() else v) for n, v in sd.items()})
    ref.gru.dropout = 0.0
    ropt = torch.optim.Adam(ref.parameters(), lr=cases.LR, weight_decay=cases.WEIGHT_DECAY)
    ref_losses = []
    for _ in range(3):
        ropt.zero_grad(set_to_none=True)
        out = ref(x.double())
        loss = sum(w[g] * F.cross_entropy(out[:, a:b], y[:, g], label_smoothing=eps) for g, (a, b) in enumerate(slots_ref.segments(FSC)))
        loss.backward()
        ropt.step()
        ref_losses.append(loss.item())
    m = _model(24, sd)
    opt = FusedAdam(m.parameters(), lr=cases.LR, weight_decay=cases.WEIGHT_DECAY)
    crit = slots.SlotLoss(FSC, w, label_smoothing=eps)
    xd, yd = x.to(DEV), y.to(DEV)
    losses = []
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        loss = crit(m(xd), yd)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    dl = np.abs(np.asarray(losses) - np.asarray(ref_losses))
    print("slot steps: losses", losses, "reference", ref_losses, "max diff", dl.max())
    assert dl.max() <= 1e-4, dl
    ops.check_status()


def test_accumulator_result_on_321_rows_in_three_uneven_updates():
    logits, ya, _, _ = slots_ref.case(FSC, 321)
    betas = slots_ref.betas_of(FSC)
    spec = slots.SlotSpec(["action", "object", "location"], [[f"a{i}" for i in range(6)], [f"o{i}" for i in range(14)], [f"l{i}" for i in range(4)]])
    acc = slots.SlotEvalAccumulator(spec, n_bins=M, inv_temperature=betas)
    ref = slots_ref.empty_state(FSC, M)
    for a, b in ((0, 100), (100, 101), (101, 321)):
        acc.update(_dev(logits[a:b]), _dev(ya[a:b]))
        slots_ref.eval_accumulate_slots(ref, logits[a:b], ya[a:b], FSC, M, betas)
    res = acc.result()
    want_joint = slots.joint_report(ref["joint"])
    j = res["joint"]
    assert set(j) >= {"n", "exact_match_accuracy", "nll", "ece", "mce", "slots_correct", "n_excluded"}
    assert j["n"] == want_joint["n"] == 319 and j["n_excluded"] == 2 and np.array_equal(j["slots_correct"], want_joint["slots_correct"])
    assert j["exact_match_accuracy"] == want_joint["exact_match_accuracy"]
    for f in ("nll", "ece", "mce"):
        assert j[f] == pytest.approx(want_joint[f], rel=1e-6, abs=1e-9), f
    for g, c in enumerate(spec.columns):
        got, want = res["slots"][c], metrics.report_from_state(ref["slots"][g])
        assert np.array_equal(got["confusion"], want["confusion"]) and got["n"] == want["n"] and got["n_ignored"] == want["n_ignored"]
        assert got["accuracy"] == want["accuracy"] and got["nll"] == pytest.approx(want["nll"], rel=1e-6)
        assert list(got["classification"])[:2] == [spec.vocab[g][0], spec.vocab[g][1]]
    # data-parallel use: two shards merged give the same report
    a1 = slots.SlotEvalAccumulator(spec, n_bins=M, inv_temperature=betas).update(_dev(logits[:150]), _dev(ya[:150]))
    a2 = slots.SlotEvalAccumulator(spec, n_bins=M, inv_temperature=betas).update(_dev(logits[150:]), _dev(ya[150:]))
    merged = a1.merge(a2.state_arrays()).result()["joint"]
    assert merged["n"] == j["n"] and np.array_equal(merged["slots_correct"], j["slots_correct"]) and merged["nll"] == pytest.approx(j["nll"], rel=1e-12)
    assert acc.reset().result()["joint"]["n"] == 0
    # per-slot temperatures: the existing fit on each segment's contiguous copy
    fitted = slots.fit_slot_temperatures(_dev(logits), _dev(ya), spec)
    assert fitted.shape == (3,) and fitted.dtype == torch.float32 and fitted.is_cuda
    for g, (a, b) in enumerate(slots_ref.segments(FSC)):
        assert torch.equal(fitted[g], metrics.fit_temperature(_dev(logits[:, a:b].contiguous()), _dev(ya[:, g].contiguous()))[0])
    slots.classify(_dev(logits), spec, inv_temperature=fitted)
    ops.check_status()


def test_result_dictionaries_and_rejection_on_the_joint_confidence():
    from sir_amd.scripts import classify_results
    spec = slots.SlotSpec(["action", "object", "location"],
                          [["activate", "bring", "change", "deactivate", "decrease", "increase"], [f"o{i}" for i in range(14)],
                           ["bedroom", "kitchen", "none", "washroom"]])
    logits = slots_ref.case(FSC, 17)[0]
    logits[4, 3] = float("nan")
    temps = [1.0, 2.0, 0.5]
    betas = [1.0, 0.5, 2.0]
    res = classify_results.results_from_slot_logits(_dev(logits), spec, k=3, inv_temperature=betas, min_confidence=0.16)
    _, ref_i, ref_t, ref_j = slots_ref.classify_slots(logits, FSC, 3, betas)
    assert len(res) == 17
    for b, r in enumerate(res):
        if b == 4:
            assert r["action"] == "Unknown" and np.isnan(r["confidence"]) and r["rejected"] is True and np.isnan(r["slot_confidence"]["action"])
            assert r["object"] == spec.vocab[1][ref_i[b, 1, 0]] and abs(r["slot_confidence"]["object"] - ref_t[b, 1, 0]) <= 4e-6
            continue
        assert [r[c] for c in spec.columns] == [spec.vocab[g][ref_i[b, g, 0]] for g in range(3)]
        assert r["predicted_label"] == f"{r['action']}_{r['object']}"                     # the reference's join
        assert abs(r["confidence"] - ref_j[b]) <= 4e-6 * 3
        assert r["rejected"] == (not (r["confidence"] >= 0.16))
        for g, c in enumerate(spec.columns):
            assert abs(r["slot_confidence"][c] - ref_t[b, g, 0]) <= 4e-6
            assert [e["label"] for e in r["top_predictions"][c]] == [spec.vocab[g][i] for i in ref_i[b, g]]
            assert len(r["top_predictions"][c]) == 3 and r["top_predictions"][c][0]["probability"] == r["slot_confidence"][c]
    flags = [r["rejected"] for r in res]
    assert any(flags) and not all(flags)                                                  # the threshold cuts through this batch
    # the callers' builder: T per slot, no threshold -> no "rejected" key; k above a width is cut to the width
    plain = classify_results.results_of(_dev(logits), {}, spec, temps, None)
    assert "rejected" not in plain[0] and plain[0]["confidence"] == res[0]["confidence"]
    wide = classify_results.results_from_slot_logits(_dev(logits), spec, k=8)
    assert [len(wide[0]["top_predictions"][c]) for c in spec.columns] == [6, 8, 4]
    assert classify_results.results_of(_dev(logits[:, :6].contiguous()), {i: str(i) for i in range(6)})[0]["predicted_label"] in map(str, range(6))


def test_validate_counts_exact_matches():
    from sir_amd.scripts.train import validate
    m = _model(24)
    x = synth.synth_features(12, 16, seed=3).to(DEV)
    with torch.no_grad():
        m.eval()
        out = m(x)
    idx, _, _ = slots.classify(out, FSC, k=1)
    y = idx[:, :, 0].to(torch.int64).clone()
    y[0, 1] = (y[0, 1] + 1) % 14                                                          # one slot of one clip wrong
    y[5, 2] = (y[5, 2] + 1) % 4
    y[7] = (y[7] + 1) % 4                                                                 # all three wrong: still one clip
    crit = slots.SlotLoss(FSC)
    loss, acc = validate(m, [(x[:8], y[:8]), (x[8:], y[8:])], crit, torch.device(DEV))
    assert acc == 9 / 12 and np.isfinite(loss)
    ops.check_status()


def test_train_and_evaluate_with_the_slots_key(tmp_path):
    from sir_amd.scripts import evaluate as ev
    from sir_amd.scripts import precompute_features as pf
    from sir_amd.scripts import train as tr
    from test_pipeline_gpu import _make_corpus

    rows = _make_corpus(str(tmp_path / "wav"))
    for i, r in enumerate(rows):
        r["action"], r["object"] = r["label"].split("_")
        r["location"] = ["kitchen", "bedroom", "none"][i % 3]
    csvs = {}
    for split, sl in (("train", slice(0, 16)), ("valid", slice(16, 24))):
        p = tmp_path / f"{split}_data.csv"
        pd.DataFrame(rows[sl]).to_csv(p, index=False)
        csvs[split] = str(p)
        pf.precompute_dataset_features(str(p), str(tmp_path / "cache"))
    spec = slots.SlotSpec.from_csv(csvs["train"])
    assert spec.sizes == (4, 2, 3)
    spec.save(str(tmp_path / "slot_map.json"))
    cfg = {"batch_size": 8, "num_workers": 0, "num_labels": 9, "lr": 1e-3, "weight_decay": 1e-4, "epochs": 1,
           "early_stop_patience": 5, "augment_prob": 0.7, "cache_dir": str(tmp_path / "cache"), "use_feature_cache": True,
           "save_path": str(tmp_path / "ckpt"), "mixup": 0.2, "label_smoothing": 0.1,
           "slots": {"map": str(tmp_path / "slot_map.json"), "weights": [1.0, 1.0, 0.5]}}
    args = types.SimpleNamespace(train_csv=csvs["train"], val_csv=csvs["valid"], label_map=None)
    best = tr.train(args, cfg)
    assert 0.0 <= best <= 1.0
    torch.save(synth.synth_state_dict(9, seed=0), str(tmp_path / "model.pt"))
    eargs = types.SimpleNamespace(test_csv=csvs["valid"], label_map=None, model_path=str(tmp_path / "model.pt"))
    with pytest.raises(ValueError, match="device_metrics"):
        ev.evaluate(eargs, cfg)
    acc = ev.evaluate(eargs, dict(cfg, device_metrics=True))
    out = tmp_path / "ckpt" / "evaluation_results"
    joint = json.load(open(out / "joint_metrics.json"))
    assert joint["n"] + joint["n_excluded"] == 8 and joint["exact_match_accuracy"] == acc and sum(joint["slots_correct"]) == joint["n"]
    for c in spec.columns:
        assert (out / f"classification_report_{c}.txt").exists() and json.load(open(out / f"calibration_{c}.json"))["n"] == 8
    # files -> slot dictionaries through predict_many: the same builder on the model's logits
    from sir_amd.scripts import predict_frontend
    m = _model(9).eval()
    paths = [rows[0]["path"], rows[1]["path"], rows[9]["path"]]                            # (the third file does not exist)
    res = predict_frontend.predict_many(m, paths, {}, torch.device(DEV), slots=spec, temperature=[1.0, 2.0, 1.0], min_confidence=0.9)
    assert res[2] is None and all(r is not None for r in res[:2])
    for r in res[:2]:
        assert set(spec.columns) <= set(r) and r["predicted_label"] == f"{r['action']}_{r['object']}" and r["action"] in spec.vocab[0]
        assert 0.0 < r["confidence"] <= 1.0 and r["rejected"] == (not (r["confidence"] >= 0.9))
        assert abs(r["confidence"] - np.prod([r["slot_confidence"][c] for c in spec.columns])) <= 4e-6 * 3
    ops.check_status()
