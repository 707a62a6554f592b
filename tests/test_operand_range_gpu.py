"""The fp16 contractions at their range edges, against the float64 oracle.

Every contraction on the hot path is an f16x3 product of fp32 operands split into two fp16 planes (csrc/f16_split.h): exact to 22-23
bits for 2^-14 <= |x| <= 65504, an ABSOLUTE 2^-36 below, clamped above, and the clamp turns a NaN into a finite number.  The
single-accumulator forms (Winograd convolutions and weight gradients, the GRU backward GEMMs) need |b| * scale < 32 on one side.
The other training tests start from synth_state_dict(seed 0) with unit-scale features and random labels (loss ~ 3.4): the one
point where every operand sits comfortably inside.  This module walks the magnitude axis; include/sir_hip.h (at sir_model_infer)
states the contract it holds the library to.  Shapes: (B, t) = (8, 200), the golden training shape, where noted; (5, 96) otherwise
-- magnitude faults do not depend on the shape.  References: tests/range_ref.py (the float64 oracle at the device's own ReLU /
max-pool values, differentiated for an arbitrary dlogits) and input_grad_ref.reference.  Bounds are _training_case's: max |a - b|
<= 2e-3 * rms per tensor, norms within 1e-3, stage gradients of the workspace (divided by the scale the device used) 2e-3 * rms.

A. The backward's gradient-magnitude window (batch statistics).  One forward, dl = (softmax - onehot) / B from sir_ce_loss,
   logits.backward(dl * 2^k); reference = the k = 0 float64 gradient * 2^k (the oracle is linear in dlogits).  fp32 softmax - onehot
   is 0 or at least ~2^-24 of O(1), so k in [-24, 0] is all a real forward can produce; k = +5, +10 is the head room the source
   used to document, k = +16 lies beyond any static scale.  The backward picks its power-of-two scale from max |dlogits|
   (bwd_scale_kernel, workspace slot 39), so every k lands on the same internal values.  Measured (worst gradient / worst norm /
   worst stage gradient): k = -24 and 0 at (8, 200) 5.7e-6 / 3.5e-7 / 5.7e-6; k = -16, -8, +5, +10, +16 at (5, 96) 5.5e-6 /
   2.6e-7 / 4.2e-6 -- identical figures for every k of a shape, as they must be.  Largest passing k on the high side: +16 (the
   largest tried; the scale follows).  The static scale 2^8 * batch is kept while max |dlogits| * scale lies in [2^5, 2^10) --
   at (5, 96) that is k in [-3, +1] -- so the band's two ends and the first k outside them are cases too: k = -3 / +1 stay static
   (asserted) with 5.9e-6 / 6.9e-6 (conv2.weight), k = -4 / +2 move (asserted) and give the 5.5e-6 of every other k.  A NaN in
   dlogits comes out as non-finite fc gradients and a non-finite total norm (measured: in all 29 gradients).  A mixed batch at (8, 200), row b
   scaled by 2^(-4 b) (2^0 ... 2^-28): worst gradient 7.3e-6 (gru.weight_hh_l0), worst norm 1.7e-7.
B. Per-row range of the input gradient (frozen statistics: explain.fgsm's path).  B = 7, t = 96, row b of dlogits scaled by
   2^(-4 b); the bound holds PER ROW, which is what makes the sign FGSM / PGD takes on a confidently classified clip trustworthy.
   Every utterance gets a scale of its own (slot 39, pair 1 + b: 2^11, 2^14, 2^18 ... 2^34).  Measured max |dx[b] - ref[b]| /
   rms(ref[b]): 3.2e-6, 2.9e-6, 2.9e-6, 3.3e-6, 2.9e-6, 2.7e-6, 3.0e-6 for rms(ref[b]) from 2.9e-5 down to 1.7e-12.
C. Non-finite values follow the oracle.  x[1,7,40] = NaN, x[2,0,0] = +Inf, x[3,63,95] = -Inf at (5, 96): the float64 oracle makes
   rows 1, 2, 3 non-finite in all 31 logits in eval mode, and the loss and all 29 gradients non-finite in training mode.
   Inference (padded and ragged): the same rows are NaN, rows 0 and 4 bit-identical to the clean batch.  Training: loss and the
   fused clip's total norm are non-finite.  Weights, per family as the header documents: a NaN in conv2.weight (bit 3),
   gru.weight_hh_l0 (bit 11), conv1.weight or bn2.weight (bit 13: before the flag both gave finite logits and a finite loss) is
   REPORTED (SIR_EINVAL at check_status, each matched by its own message), a NaN in fc.weight[3, 3] comes out as column 3 of the
   logits, as in the oracle.  Every model here is built for its test and dies with it (its prepared weights live
   in its own workspace under its own token), and the status word is read back clean before the test ends.
D. Stated operand limits.  conv2.weight[0,0,0,0] = 40 (U corner 40 >= 32): status bit 3 in inference and training.
   conv2.weight[0,0,1,1] = 40 (|U| <= 10) and a corner of 20: no flag, parity.  bn1 / bn2.bias[5] = 100 with gamma 1 (a1 / a2 up
   to ~105, inside 256): parity, worst gradient 5.6e-5 (conv2.weight) / 4.1e-5 (conv3.weight).  bn2.bias = 300 (conv3 weight-gradient input beyond 256; a fixed scale would
   give 0.33 * rms on conv3.weight) and bn3.bias = 600 (GRU weight-gradient b side beyond 512; 34 * rms on gru.weight_ih_l0):
   status bit 12 from the training forward.  Trained-scale weights (gru.* x 4 and x 8, BatchNorm gammas x 2, fc.* x 8: saturated
   gates).  Inference bound = max(2e-5, 2 x the float32 oracle's own distance from float64 on the same inputs) -- the factor 2 is
   what test_features_gpu.py grants a path that sums in another order; the measure is the reference's error, never the device's.
   Gradient bound likewise per tensor: max(2e-3, 2 x the float32 oracle's error at the same overridden forward values); the norms
   keep their 1e-3 (the float32 oracle's worst norm error is 7.6e-7 / 7.7e-6 at x4 / x8, 2.3e-7 in the conv cases: no room needed).
   Measured, x4 / x8: eval logits rms 2.14 / 2.34; float32 oracle vs float64 9.8e-6 / 3.0e-5, device 7.2e-6 / 1.6e-5; gradients:
   float32 oracle 5.6e-5 / 1.1e-3 * rms (gru.weight_ih_l0_reverse), device 4.7e-5 / 5.9e-4; the norm of attention.bias's gradient,
   zero in exact arithmetic, is 8.8e-8 / 6.7e-8 in the float32 oracle and gets 2 x that as its absolute term (_training_case's
   norm_atol rule; device 1.1e-7 at x8).  Not x16: the float32 oracle itself
   is at 1.9e-3 there and the case says nothing.

Every case prints what it asserts on first, and ends in ops.check_status() unless it expects that call to raise."""
import functools

import pytest
import torch

import cases
import input_grad_ref
import range_ref
from oracle import model_ref
from sir_amd import _native, explain, ops, synth, train_ops
from sir_amd.models.models import CNNAudioGRU
from train_step_ref import _device_forward_values, _loss_scale, _rel, _views

pytestmark = pytest.mark.gpu
DEV = "cuda"
NCLS = 31
SMALL, GOLDEN = (5, 96), (8, 200)


def _sd():
    return synth.synth_state_dict(NCLS, seed=0)


def _model(sd, train):
    m = CNNAudioGRU(NCLS)
    m.load_state_dict(sd)
    m = m.to(DEV)
    m.train(train)
    m.gru.dropout = 0.0
    return m


def _inputs(bsz, t):
    """The inputs of ``train_step_ref._training_case`` at this shape."""
    return cases.varied_features(bsz, t, seed=3000 + bsz), synth.synth_labels(bsz, NCLS, seed=3001 + bsz)


def _ce_dlogits(logits, y):
    """``(loss, d loss / d logits)`` of the mean cross-entropy by ``sir_ce_loss``: ``(softmax - onehot) / B``."""
    lg = logits.detach().requires_grad_(True)
    loss = train_ops.fused_cross_entropy(lg, y.to(DEV))
    (dl,) = torch.autograd.grad(loss, lg)
    return loss.detach(), dl


class _Step:
    """One training-mode forward of ``sd`` at ``(bsz, t)`` on the device (kept: ``backward(dlogits)`` may run many times on it)
    and the float64 oracle at the device's own z / y values."""

    def __init__(self, sd, bsz, t, x=None):
        self.sd, self.bsz, self.t = sd, bsz, t
        self.x, self.y = _inputs(bsz, t)
        if x is not None:
            self.x = x
        self.m = _model(sd, train=True)
        self.logits = self.m(self.x.to(DEV))
        self.loss, self.dl = _ce_dlogits(self.logits, self.y)
        torch.cuda.synchronize()
        self.views = lambda: _views(self.m, bsz, t)
        self.zo, self.yo = _device_forward_values(self.m, sd, self.x, bsz, t, self.views())
        self.oracle = range_ref.TrainOracle(sd, self.x, self.zo, self.yo)

    def backward(self, dlogits):
        self.m.zero_grad(set_to_none=True)
        self.logits.backward(dlogits.contiguous(), retain_graph=True)
        torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def _window_step(shape):
    s = _Step(_sd(), *shape)
    s.ref_grads, s.ref_stages = s.oracle.vjp(s.dl)            # k = 0; the oracle is linear in dlogits
    return s


# ---- A. gradient-magnitude window of the training backward ------------------------------------------------------------------
def _window_case(k, shape):
    s = _window_step(shape)
    s.backward(s.dl * 2.0 ** k)
    scale = range_ref.device_loss_scale(s.m, s.bsz, s.t)
    print(f"k={k} B={s.bsz} t={s.t}: max|dlogits| = {(s.dl * 2.0 ** k).abs().max().item():.2e}, device loss scale 2^"
          f"{torch.tensor(scale).log2().item():.0f} (static 2^{torch.tensor(_loss_scale(s.bsz)).log2().item():.0f})")
    gerr, nerr, serr = range_ref.backward_errors(s.m, s.ref_grads, 2.0 ** -k, s.views(), s.ref_stages, scale * 2.0 ** k)
    return s, scale, (gerr, nerr, serr)


# at (5, 96) max |dl| * 2^11 lies in [2^8, 2^9): the static scale is kept for k in [-3, +1], the band's two ends, and left at -4 / +2
STATIC_BAND = (-3, 1)


@pytest.mark.parametrize("k,shape", [(-24, GOLDEN), (-16, SMALL), (-8, SMALL), (-4, SMALL), (-3, SMALL), (0, GOLDEN), (1, SMALL), (2, SMALL),
                                     (5, SMALL), (10, SMALL)])
def test_backward_window(k, shape):
    """``logits.backward(dl * 2^k)`` against the k = 0 float64 gradient times 2^k: all 29 gradients and the five stage gradients."""
    s, scale, errs = _window_case(k, shape)
    range_ref.assert_backward(f"k={k}", *errs)
    if STATIC_BAND[0] <= k <= STATIC_BAND[1]:
        assert scale == _loss_scale(s.bsz)                   # a mean cross-entropy, and 2^-3 .. 2^1 of it, sits on the static scale
    else:
        assert scale == _loss_scale(s.bsz) * 2.0 ** -k * (1.0 if shape == GOLDEN else 0.5)   # scaled maximum back in [2^7, 2^8)
    ops.check_status()


def test_backward_far_above_window():
    """k = +16: never finite and wrong."""
    s, scale, errs = _window_case(16, SMALL)
    try:
        ops.check_status()
    except _native.SirError as e:
        print("k=16: check_status raised:", e)
        return
    finite = all(torch.isfinite(p.grad).all().item() for p in s.m.parameters())
    print(f"k=16: check_status clean, gradients finite: {finite}")
    if finite:
        range_ref.assert_backward("k=16", *errs)


def test_backward_mixed_rows():
    """Row b of dlogits scaled by 2^(-4 b) at the golden shape: the small rows do not disturb the sums the large rows dominate."""
    s = _window_step(GOLDEN)
    dl = s.dl * (2.0 ** (-4.0 * torch.arange(s.bsz, device=DEV)))[:, None]
    ref_grads, _ = s.oracle.vjp(dl)
    s.backward(dl)
    gerr, nerr, _ = range_ref.backward_errors(s.m, ref_grads)
    range_ref.assert_backward("mixed rows 2^0 .. 2^-28", gerr, nerr, {})
    ops.check_status()


def test_backward_nonfinite_dlogits():
    """A NaN in dlogits: the fc gradients come from dlogits in fp32 and are non-finite, and with them the clip's total norm -- what a
    training loop looks at.  (The other gradients pass f16 splits that clamp and are unspecified: include/sir_hip.h.)"""
    s = _window_step(SMALL)
    dl = s.dl.clone()
    dl[0, 0] = float("nan")
    s.backward(dl)
    total = train_ops.clip_grad_norm_(list(s.m.parameters()), 1.0)
    bad = {n: int((~torch.isfinite(p.grad)).sum()) for n, p in s.m.named_parameters()}
    print("non-finite gradient elements per tensor:", {n: c for n, c in bad.items() if c}, "total norm", total.item())
    assert bad["fc.weight"] > 0 and bad["fc.bias"] > 0
    assert not torch.isfinite(total).item()
    ops.check_status()


# ---- B. per-row range of the input gradient -----------------------------------------------------------------------------------
def test_input_gradient_rows_of_mixed_magnitude():
    bsz, t = 7, 96
    sd = _sd()
    x, y = _inputs(bsz, t)
    m = _model(sd, train=False)
    logits, leaf = explain._forward(m, x.to(DEV))
    _, dl = _ce_dlogits(logits, y)
    dl = dl * (2.0 ** (-4.0 * torch.arange(bsz, device=DEV)))[:, None]
    (dx,) = torch.autograd.grad(logits, leaf, grad_outputs=dl.contiguous())
    torch.cuda.synchronize()
    zo, yo = input_grad_ref.device_forward_values(m, sd, x, bsz, t)
    _, _, ref_dx = input_grad_ref.reference(sd, x, zo, yo, bn_frozen=(True,) * 3, dlogits=dl)
    ratios = [input_grad_ref.ratio(dx[b], ref_dx[b]) for b in range(bsz)]
    scales = [range_ref.device_loss_scale(m, bsz, t, row=b) for b in range(bsz)]
    print("per-row max|dx - ref| / rms(ref):", [f"{r:.1e}" for r in ratios], "rms(ref):",
          [f"{ref_dx[b].pow(2).mean().sqrt().item():.1e}" for b in range(bsz)], "row scales 2^", [int(torch.tensor(v).log2()) for v in scales])
    for b, r in enumerate(ratios):
        assert r <= input_grad_ref.GRAD_BOUND, (b, r)
    ops.check_status()


# ---- C. non-finite values follow the oracle -----------------------------------------------------------------------------------
BAD = [((1, 7, 40), float("nan")), ((2, 0, 0), float("inf")), ((3, 63, 95), float("-inf"))]
RAGGED_LENGTHS = [96, 48, 96, 96, 64]                          # the three elements stay inside their clips


def _bad_features():
    x, y = _inputs(*SMALL)
    bad = x.clone()
    for idx, v in BAD:
        bad[idx] = v
    return x, bad, y


@pytest.mark.parametrize("lengths", [None, RAGGED_LENGTHS], ids=["padded", "ragged"])
def test_nonfinite_features_cost_their_own_rows_in_inference(lengths):
    sd = _sd()
    x, bad, _ = _bad_features()
    with torch.no_grad():
        ref = model_ref.forward({k: v.double() if v.is_floating_point() else v for k, v in sd.items()}, bad.double())
    ref_bad = ~torch.isfinite(ref)
    print("oracle: non-finite logits per row", ref_bad.sum(1).tolist())
    assert ref_bad.all(1).tolist() == [False, True, True, True, False] and ref_bad.any(1).tolist() == ref_bad.all(1).tolist()
    m = _model(sd, train=False)
    clean, _ = m.predict(x.to(DEV), lengths=lengths)
    got, _ = m.predict(bad.to(DEV), lengths=lengths)
    got_bad = ~torch.isfinite(got).cpu()
    same = [torch.equal(got[b], clean[b]) for b in range(SMALL[0])]
    print("device: non-finite logits per row", got_bad.sum(1).tolist(), "rows bit-identical to the clean batch", same)
    assert torch.equal(got_bad, ref_bad)
    assert same == [True, False, False, False, True]
    ops.check_status()


def test_nonfinite_features_make_the_training_loss_nonfinite():
    sd = _sd()
    _, bad, y = _bad_features()
    ref_loss, ref_grads, _, _ = model_ref.loss_and_grads({k: v.double() if v.is_floating_point() else v for k, v in sd.items()}, bad.double(), y)
    assert not torch.isfinite(ref_loss) and all(not torch.isfinite(g).any() for g in ref_grads.values())
    m = _model(sd, train=True)
    logits = m(bad.to(DEV))
    loss = train_ops.fused_cross_entropy(logits, y.to(DEV))
    loss.backward()
    total = train_ops.clip_grad_norm_(list(m.parameters()), 1.0)
    print(f"oracle loss {ref_loss.item()}, device loss {loss.item()}, total gradient norm {total.item()}, finite logits "
          f"{int(torch.isfinite(logits).sum())} of {logits.numel()}")
    assert not torch.isfinite(loss).item()                     # what a caller's isfinite(loss) check sees
    assert not torch.isfinite(total).item()
    ops.check_status()


WEIGHT_CASES = [("conv2.weight", (0, 0, 0, 0), r"\|U\| >= 32"), ("gru.weight_hh_l0", (5, 5), "GRU weight matrix"), ("fc.weight", (3, 3), "follows"),
                ("conv1.weight", (0, 0, 0, 0), "conv1 weight or a BatchNorm"), ("bn2.weight", (5,), "conv1 weight or a BatchNorm")]


@pytest.mark.parametrize("train", [False, True], ids=["infer", "train"])
@pytest.mark.parametrize("name,idx,how", WEIGHT_CASES, ids=[c[0] for c in WEIGHT_CASES])
def test_nonfinite_weight(name, idx, how, train):
    """include/sir_hip.h, per weight family: a non-finite convolution or GRU matrix is REPORTED (the weight-preparation kernels
    raise the status word: SIR_EINVAL at the next check, matched here by its own message); fc / attention travel in fp32 and come
    out where the oracle has them; a NaN in conv1.weight or a BatchNorm parameter sits in front of an fmaxf ReLU / max-pool that
    drops it (finite logits and loss were measured before the flag existed) and is reported by the kernels that fold those
    parameters: status bit 13."""
    sd = dict(_sd())
    sd[name] = sd[name].clone()
    sd[name][idx] = float("nan")
    x, y = _inputs(*SMALL)
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
    with torch.no_grad():
        ref_bad = ~torch.isfinite(model_ref.forward(sd64, x.double(), train=train))
    print(f"{name} {'train' if train else 'infer'}: oracle non-finite logits per column", ref_bad.sum(0).tolist())
    assert ref_bad.all(0).tolist() == ref_bad.any(0).tolist()
    assert ref_bad[:, 3].all() and (ref_bad.all() or name == "fc.weight")
    m = _model(sd, train=train)                                # (a model of its own: its prepared weights die with it)
    if train:
        logits = m(x.to(DEV))
        loss = train_ops.fused_cross_entropy(logits, y.to(DEV))
        loss.backward()
    else:
        logits, _ = m.predict(x.to(DEV))
    got_bad = ~torch.isfinite(logits.detach()).cpu()
    print(f"device non-finite logits per column", got_bad.sum(0).tolist(), f"loss {loss.item()}" if train else "")
    if how != "follows":
        with pytest.raises(_native.SirError, match="code -1.*" + how):
            ops.check_status()
    else:
        assert torch.equal(got_bad, ref_bad)
        if train:
            assert not torch.isfinite(loss).item()
        ops.check_status()
    ops.check_status()                                         # (the word was cleared: nothing is left for the neighbours)


# ---- D. stated operand limits: exact inside, reported outside -----------------------------------------------------------------
def _f64(sd):
    return {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}


def _inference_vs_oracles(tag, sd):
    """Device eval logits against the float64 oracle; the bound is max(2e-5, 2 x the float32 oracle's own distance from it)."""
    x, _ = _inputs(*SMALL)
    with torch.no_grad():
        ref = model_ref.forward(_f64(sd), x.double())
        own = (model_ref.forward(sd, x).double() - ref).abs().max().item()
    m = _model(sd, train=False)
    got, _ = m.predict(x.to(DEV))
    err = (got.cpu().double() - ref).abs().max().item()
    bound = max(2e-5, 2.0 * own)
    print(f"{tag} inference: logits rms {ref.pow(2).mean().sqrt().item():.2f}, float32 oracle vs float64 {own:.1e}, device vs float64 "
          f"{err:.1e}, bound {bound:.1e}")
    assert err <= bound
    return own, err


def _training_vs_oracles(tag, sd, f32_bound):
    """One training step's 29 gradients against the float64 oracle at the device's forward values.  ``f32_bound``: per tensor
    max(2e-3, 2 x the float32 oracle's error at the same values) instead of 2e-3."""
    s = _Step(sd, *SMALL)
    ref_grads, ref_stages = s.oracle.vjp(s.dl)
    bound = norm_bound = norm_atol = None
    if f32_bound:
        g32, _ = range_ref.TrainOracle(sd, s.x, s.zo, s.yo, dtype=torch.float32).vjp(s.dl)
        own = {k: _rel(g32[k], ref_grads[k])[0] for k in g32 if ref_grads[k].abs().max() > 1e-7}
        own_n = {k: abs(g32[k].double().norm().item() / ref_grads[k].norm().item() - 1.0) for k in own}
        worst = max(own, key=own.get)
        print(f"{tag}: float32 oracle vs float64 oracle: worst gradient {own[worst]:.1e} * rms ({worst}), worst norm {max(own_n.values()):.1e}")
        bound = {k: max(range_ref.GRAD_BOUND, 2.0 * e) for k, e in own.items()}     # (the norms keep their 1e-3: the float32 oracle's
                                                                                    # own norm error, printed above, is far inside it)
        # a gradient that is zero in exact arithmetic (attention.bias: the softmax ignores a shift): the absolute term of its
        # norm bound is 2 x what the float32 oracle leaves there, where that exceeds the 1e-7 of _training_case
        norm_atol = {k: max(1e-7, 2.0 * g32[k].double().norm().item()) for k in g32 if k not in own}
        for k, a in norm_atol.items():
            print(f"{tag}: |{k} gradient| (zero in exact arithmetic): float32 oracle {g32[k].double().norm().item():.2e}, float64 oracle "
                  f"{ref_grads[k].norm().item():.2e}, absolute bound {a:.2e}")
    s.backward(s.dl)
    lerr = (s.logits.detach().cpu().double() - s.oracle.logits.detach()).abs().max().item()
    print(f"{tag}: loss {s.loss.item():.3f}, training logits vs float64 {lerr:.1e}")
    scale = range_ref.device_loss_scale(s.m, s.bsz, s.t)
    errs = range_ref.backward_errors(s.m, ref_grads, 1.0, s.views(), ref_stages, scale)
    return s, errs, dict(bound=bound, norm_bound=norm_bound, norm_atol=norm_atol)


def _with(sd, edits):
    sd = dict(sd)
    for name, idx, v in edits:
        sd[name] = sd[name].clone()
        sd[name][idx] = v
    return sd


@pytest.mark.parametrize("train", [False, True], ids=["infer", "train"])
def test_conv_weight_beyond_the_limit_is_reported(train):
    """conv2.weight[0,0,0,0] = 40: the corner of U = G g G^T is 40 >= 32 -> status bit 3."""
    sd = _with(_sd(), [("conv2.weight", (0, 0, 0, 0), 40.0)])
    x, y = _inputs(*SMALL)
    m = _model(sd, train=train)
    if train:
        train_ops.fused_cross_entropy(m(x.to(DEV)), y.to(DEV)).backward()
    else:
        m.predict(x.to(DEV))
    with pytest.raises(_native.SirError, match=r"code -1.*\|U\| >= 32"):
        ops.check_status()
    ops.check_status()


@pytest.mark.parametrize("idx,v", [((0, 0, 1, 1), 40.0), ((0, 0, 0, 0), 20.0)], ids=["centre40", "corner20"])
def test_conv_weight_inside_the_limit_holds_parity(idx, v):
    sd = _with(_sd(), [("conv2.weight", idx, v)])
    _inference_vs_oracles(f"conv2.weight{list(idx)}={v:g}", sd)
    ops.check_status()
    s, errs, bounds = _training_vs_oracles(f"conv2.weight{list(idx)}={v:g}", sd, f32_bound=True)
    range_ref.assert_backward(f"conv2.weight{list(idx)}={v:g} training", *errs, **bounds)
    ops.check_status()


ACT_CASES = [("bn1", 100.0, True), ("bn2", 100.0, True), ("bn2", 300.0, False), ("bn3", 600.0, False)]


@pytest.mark.parametrize("bn,bias,inside", ACT_CASES, ids=[f"{c[0]}.bias={c[1]:g}" for c in ACT_CASES])
def test_activation_limits(bn, bias, inside):
    """One channel of a BatchNorm pushed up by its bias (gamma 1): a1 / a2 up to 100 is inside the conv2 / conv3 weight gradient's
    256 and the GRU weight-gradient GEMMs' 512; a2 = 300 / x0 = 600 is beyond one of them -- parity all the same, or a report."""
    c = 5
    sd = _with(_sd(), [(f"{bn}.weight", (c,), 1.0), (f"{bn}.bias", (c,), bias)])
    tag = f"{bn}.bias[{c}]={bias:g}"
    s, errs, _ = _training_vs_oracles(tag, sd, f32_bound=False)
    v = s.views()
    print(f"{tag}: max a1 {v['a1'].max().item():.1f}, max a2 {v['a2'].max().item():.1f}, max x0 {v['x0'].max().item():.1f}")
    if inside:
        range_ref.assert_backward(tag, *errs)
        ops.check_status()
        return
    try:
        ops.check_status()
    except _native.SirError as e:
        print(f"{tag}: check_status raised:", e)
        assert "code -1" in str(e)
        return
    range_ref.assert_backward(tag, *errs)


@pytest.mark.parametrize("gain", [4.0, 8.0])
def test_trained_scale_weights(gain):
    """gru.* x gain, BatchNorm gammas x 2, fc.* x 8: saturated gates, the tails of the sigmoid / tanh."""
    sd = dict(_sd())
    for k in sd:
        if k.startswith("gru."):
            sd[k] = sd[k] * gain
        elif k.startswith("fc."):
            sd[k] = sd[k] * 8.0
        elif k in ("bn1.weight", "bn2.weight", "bn3.weight"):
            sd[k] = sd[k] * 2.0
    tag = f"gru x{gain:g}"
    _inference_vs_oracles(tag, sd)
    ops.check_status()
    s, errs, bounds = _training_vs_oracles(tag, sd, f32_bound=True)
    range_ref.assert_backward(tag + " training", *errs, **bounds)
    ops.check_status()
