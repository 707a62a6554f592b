"""Every class count from 1 to 64 against the float64 oracle: the axis ``num_classes`` of sir_model_infer, sir_model_infer_ragged,
sir_model_train_fwd*, sir_model_train_bwd*, sir_ce_loss and sir_ce_loss_soft, which accept 1 <= C <= 64.  The rest of the suite runs
the model at C = 31 (and 5 / 6 without the training oracle) and the loss against a reference at 6 and 31 only.

CS = 1, 2, 32, 33, 63, 64.  What each lands on:

    C    attention_pool_body (j = tid >> 3; j < C; j += 32)        ce_loss_kernel   bwd_scale_kernel, per row   head_bwd_kernel grid
    1    one 8-lane group of the first trip, lg[0] alone           <32, .>          lane 0 of the wave          B + 2
    2    two groups of the first trip                              <32, .>          lanes 0..1                  B + 4
    32   a full first trip, no second one                          <32, .>          lanes 0..31                 B + 64
    33   a full first trip + a second with ONE group (j = 32)      <64, .>          lanes 0..32                 B + 66
    63   a second trip with one group idle (tid >= 248)            <64, .>          lanes 0..62                 B + 126
    64   both trips full: every lane and every lg[] slot live      <64, .>          the whole wave              B + 128

32 | 33 are the two sides of the loss dispatch (train_loss_optim.hip: CMAX = 32 up to 32 classes, 64 above) and of the head loop's
second trip; 63 | 64 a second trip with one group idle and with none.  The three __shfl_xor of the head loop stay inside an
8-lane group, whose lanes share j: a partly active trip reduces over active lanes only.  No ``dbg`` bits, no environment switches;
every shape is at most 300 loss rows, 17 clips and 24 frames; every case prints its figures before it asserts.

Bounds, all taken from the neighbours and none restated wider:

  1. Loss alone: test_recipe_gpu.py::test_soft_loss_and_gradient_vs_float64's two -- loss within 1e-5 absolute, each dlogits element
     within (C + 8 + R) * 2^-24 / n_valid (R = max - min of the row's logits; derived there from the kernel's operation count, C
     is a term of it) -- against recipe_ref.soft_ce.  At C = 1 with hard targets the loss is exactly 0.0 and every dlogits element
     exactly zero (expf(0) = 1, den = 1, 1 * 1 - 1 = 0).
  2. Inference: dense logits within 2e-5 of model_ref.forward in float64 (test_model_gpu.py / test_token_range_gpu.py, init-scale
     weights), context vectors within test_model_gpu.py's stage bound 1e-4 * max(1, |b|); ragged logits within 2e-4
     (test_ragged_infer_gpu.py); the arg-max identical to the oracle's wherever the oracle's top-2 margin is >= 1e-3.  The float64
     margins of these five clips are >= 4.0e-3 at every C of CS in the dense call (5.3e-3, 5.2e-3, 1.1e-1, 1.4e-2, 4.0e-3 at C = 2,
     32, 33, 63, 64) and >= 1.2e-3 in the ragged one (its clips are shorter): 0 clips are excluded, which is asserted.  A rotation of
     the head's rows permutes the logits and keeps the margins.
  3. Training: train_step_ref._training_case's own -- loss 2e-5, logits 5e-5, 29 gradients and five stage gradients 2e-3 * rms,
     norms 1e-3, BN running statistics rtol 1e-4, the input gradient input_grad_ref.GRAD_BOUND.  On top, the classifier's gradient
     row by row: the project's gradient bound applied to one class's weights, max |a - b| <= 2e-3 * rms(row of the reference) for
     fc.weight and 2e-3 * |reference| for fc.bias (a bias element is sum_b (p_bj - onehot_bj) / B: a whole number of labels against a sum
     of probabilities near B / C, about 1 / C for an unlabelled class -- no cancellation the bound would have to allow for; the test
     prints the smallest |reference|).
     At C = 1 every gradient is zero in exact arithmetic AND on the device (dlogits = 0 exactly, and every product and sum behind
     it is of zeros): exact zeros are asserted, -0.0 accepted.
  4. A head swapped on a live model: section 2's dense bound; the classifier's gradients 2e-3 * rms.

Measured on an MI355X:

    C    loss err  logits err  worst gradient  worst norm  worst stage  dfeats    fc row    CE err / bound   dense      ragged
                               (* rms)                     (* rms)      (* rms)   (* rms)   (worst of 8)     logits     logits
    1    0 exact   9.4e-8      0 exact         -           -            0 exact   0 exact   0.111            3.7e-8     4.3e-8
    2    3.0e-8    5.5e-8      1.5e-5          3.6e-7      3.8e-6       -         6.6e-7    0.192            5.6e-8     5.6e-8
    32   4.6e-8    8.5e-8      1.0e-5          3.9e-7      4.0e-6       -         8.2e-7    0.093            7.0e-8     7.0e-8
    33   3.8e-7    8.0e-8      9.8e-6          1.5e-7      3.5e-6       3.7e-6    8.4e-7    0.091            7.4e-8     7.4e-8
    63   2.9e-7    8.5e-8      9.5e-6          2.2e-7      4.3e-6       -         8.3e-7    0.067            8.3e-8     8.0e-8
    64   5.3e-7    8.5e-8      8.6e-6          2.4e-7      4.1e-6       4.2e-6    7.9e-7    0.070            8.3e-8     7.0e-8
    33   7.5e-8    1.2e-7      1.1e-5          1.7e-7      4.2e-6       -         9.9e-7    (dropout 0.5)
    64   3.5e-8    1.3e-7      1.1e-5          1.4e-7      5.0e-6       -         9.4e-7    (dropout 0.5)
    33   5.0e-8    1.0e-7      1.3e-5          1.4e-7      4.1e-6       -         1.9e-6    (17 clips of 8 frames)
    64   3.4e-7    1.1e-7      1.4e-5          1.8e-7      4.0e-6       -         1.7e-6    (17 clips of 8 frames)

(Rows without a note: 5 clips of 24 frames; "fc row" is the worse of the fc.weight rows and the fc.bias elements; the inference columns
are the worst over every head of that class count -- 1 at C = 1, 5 at C = 2, up to 11 above 32 classes.)  The float32 oracle's own worst
gradient against the float64 one at these shapes is 8.8e-6 .. 1.5e-5 * rms: the device is as close to the float64 oracle as float32
arithmetic is.  The dense context vectors are within 2.0e-7.  The input gradient under frozen statistics with supplied dlogits: 5.1e-6
and 4.5e-6 * rms over the batch at C = 33 and 64, at most 3.3e-6 for a clip on its own rms.  The smallest |reference| of an fc.bias
element is 1.1e-2 (C = 63, 64).  A head swapped in on the live model: eval logits 7.4e-8 (64 classes) and 2.0e-8 (1 class), the
classifier's gradients 4.3e-6 / 1.4e-7 * rms at 64 classes and exact zeros at 1.  The whole module takes 5 s.

Checked by hand against three wrong libraries (scratch builds, not committed): ``j += 64`` in attention_pool_body fails every
inference case and every training case above 32 classes, the frozen-statistics cases, the head swap and the bit comparison behind the
refused 65-class calls (19 tests); ``lane < min(C, 32)`` in bwd_scale_kernel fails
test_frozen_statistics_input_gradient_with_supplied_dlogits[33] and [64] and nothing else; ``CMAX = 32`` for every class count fails all
24 loss cases above 32 classes, every training case there and the head swap (34 tests).
"""
import pytest
import torch

import cases
import input_grad_ref
import mutation_ref as mr
import recipe_ref
from oracle import model_ref
from sir_amd import _native, explain, ops, synth, train_ops
from sir_amd.featurizer import get_featurizer
from sir_amd.models.models import CNNAudioGRU
from train_step_ref import _rel, _training_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24                     # unit roundoff of fp32 (round to nearest)
CS = [1, 2, 32, 33, 63, 64]
DENSE_TOL, CTX_TOL = 2e-5, 1e-4
RAGGED_TOL, MARGIN = 2e-4, 1e-3
LENGTHS = [24, 23, 16, 9, 8]
ROW_BOUND = 2e-3


def _f64(sd):
    return {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in sd.items()}


def _dev(t):
    return None if t is None else t.to(DEV)


_sds = {}


def _sd(c):
    if c not in _sds:
        _sds[c] = synth.synth_state_dict(c, seed=0)
    return _sds[c]


# ---- 1. cross-entropy alone ----------------------------------------------------------------------------------------------------
def _ce_case(c, bsz, second):
    """recipe_ref.loss_case with labels forced into rows 0, 1, 3, 4: 0 and C - 1 always, above 32 classes also 32 and 31 (row 4 is
    the ignored last row at B = 5: it is labelled then, row 2 stays ignored); with ``second`` above 32 classes row 0 has ya = 0 <
    32 <= yb = C - 1 under lam = 0 and row 4 ya = 31 < 32 = yb under a drawn lam; row 3 keeps both labels on one class."""
    logits, ya, yb, lam = recipe_ref.loss_case(bsz, c, second, seed=17 * bsz + c)
    for row, label in zip((0, 1, 3, 4), [0, c - 1] + ([32, 31] if c > 32 else [])):
        ya[row] = label
    if second:
        yb[3] = ya[3]
        if c > 32:
            yb[0], yb[4] = c - 1, 32
    return logits, ya, yb, lam


@pytest.mark.parametrize("second", [False, True])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("bsz", [5, 300])
@pytest.mark.parametrize("c", CS)
def test_loss_and_gradient_vs_float64(c, bsz, eps, second):
    """B = 300: 44 threads take a second row.  Hard targets (no second label, eps = 0) run ce_loss_kernel<., false>, the rest <., true>."""
    logits, ya, yb, lam = _ce_case(c, bsz, second)
    valid = ya[ya != -100]
    assert {0, c - 1} <= set(valid.tolist()) and (c <= 32 or {31, 32} <= set(valid.tolist()))
    assert not (second and c > 32) or bool(((ya >= 0) & (ya < 32) & (yb >= 32) & (yb < c)).any())
    lg = logits.to(DEV).requires_grad_(True)
    loss = train_ops.fused_cross_entropy(lg, _dev(ya), _dev(yb), _dev(lam), label_smoothing=eps)
    loss.backward()
    ref_loss, ref_d = recipe_ref.soft_ce(logits, ya, yb, lam, eps)
    n_valid = int((ya != -100).sum())
    err = abs(loss.item() - ref_loss.item())
    spread = (logits.max(dim=1).values - logits.min(dim=1).values).double()[:, None]
    bound = (c + 8 + spread) * U / n_valid
    derr = (lg.grad.cpu().double() - ref_d).abs()
    print(f"CE C={c} B={bsz} eps={eps} second={second}: |loss - ref| {err:.3e}, max dlogits err / bound {(derr / bound).max().item():.3f}")
    assert torch.isfinite(lg.grad).all()
    assert err <= 1e-5
    assert (derr <= bound).all()
    assert (lg.grad[ya.to(DEV) == -100] == 0).all()
    if c == 1 and not second and eps == 0.0:
        assert loss.item() == 0.0
        assert torch.count_nonzero(lg.grad).item() == 0
    ops.check_status()


@pytest.mark.parametrize("which", ["ya", "yb"])
@pytest.mark.parametrize("c", [32, 33, 64])
def test_label_equal_to_the_class_count_is_flagged(c, which):
    """The first label one past the range (through the hard kernel) and, separately, the second (through the soft one), in the
    last row: a NaN loss, the "label outside" error at the next status check, a clean status after it."""
    logits, ya, yb, lam = _ce_case(c, 5, which == "yb")
    ops.check_status()
    if which == "ya":
        ya[4] = c
    else:
        ya[4], yb[4] = 0, c
    loss = train_ops.fused_cross_entropy(logits.to(DEV).requires_grad_(True), _dev(ya), _dev(yb), _dev(lam),
                                         label_smoothing=0.1 if which == "yb" else 0.0)
    print(f"C={c} {which}[4] = {c}: loss {loss.item()}")
    assert torch.isnan(loss).item()
    with pytest.raises(_native.SirError, match="label outside"):
        ops.check_status()
    ops.check_status()


# ---- 2. inference, dense and ragged ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def infer_ref():
    """The five clips and the float64 oracle's context vectors, dense and clip by clip at LENGTHS, computed once: synth_state_dict
    draws the classifier last, so every class count shares everything below it (asserted), and the oracle's logits for any head are
    that head on these vectors."""
    x = cases.varied_features(5, 24, seed=3005).float()
    sd64 = _f64(_sd(64))
    for c in CS:
        for k, v in _sd(c).items():
            assert k in ("fc.weight", "fc.bias") or torch.equal(v, _sd(64)[k]), (c, k)
    ctx = {}
    with torch.no_grad():
        st = {}
        model_ref.forward(sd64, x.double(), stages=st)
        ctx["dense"] = st["ctx"]
        rows = []
        for b, f in enumerate(LENGTHS):
            st = {}
            model_ref.forward(sd64, x[b:b + 1, :, :f].double(), stages=st)
            rows.append(st["ctx"])
        ctx["ragged"] = torch.cat(rows)
    return x, ctx


def _heads(c, weight, bias, winner):
    """(name, fc.weight, fc.bias, tie) of every head of one class count: the initial one; its rows rotated so that clip 0's winning
    class lands on 0, on C - 1 and above 32 classes on 31 and on 32; and, for pairs (p, k), the winner rotated to p and its row and
    bias copied onto k -- k above and below the winner, above 32 classes also across 32."""
    yield "init", weight, bias, None
    if c == 1:
        return
    top = min(40, c - 1)
    for p in dict.fromkeys([0, c - 1] + ([31, 32] if c > 32 else [])):
        r = (p - winner) % c
        yield f"winner on {p}", weight.roll(r, 0), bias.roll(r, 0), None
    pairs = [(0, c - 1), (c - 1, 0)]
    if c > 32:
        pairs += [(31, 32), (32, 31), (5, top), (top, 5)]
    elif c > 2:
        pairs += [(10, 20), (20, 10)]
    for p, k in pairs:
        r = (p - winner) % c
        w, b = weight.roll(r, 0).clone(), bias.roll(r, 0).clone()
        w[k], b[k] = w[p], b[p]
        yield f"tie {p} = {k}", w, b, (p, k)


def _margin(ref):
    top2 = ref.topk(2, dim=1).values
    return top2[:, 0] - top2[:, 1]


@pytest.mark.parametrize("mode", ["dense", "ragged"])
@pytest.mark.parametrize("c", CS)
def test_inference_vs_oracle(infer_ref, c, mode):
    x, ctx = infer_ref
    ctx64 = ctx[mode]
    sd = _sd(c)
    m = CNNAudioGRU(c)
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    winner = int((ctx64[:1] @ sd["fc.weight"].double().t() + sd["fc.bias"].double()).argmax(1))
    tol = DENSE_TOL if mode == "dense" else RAGGED_TOL
    if mode == "ragged":
        xin = torch.full_like(x, float("nan"))
        for b, f in enumerate(LENGTHS):
            xin[b, :, :f] = x[b, :, :f]
        lengths = torch.tensor(LENGTHS, dtype=torch.int32, device=DEV)
        ws = ops.Workspace()
        need = _native.lib().sir_model_workspace_bytes(get_featurizer().handle, 5, 24, 0)
    else:
        xin = x
    xd = xin.to(DEV)
    worst, landed = 0.0, set()
    for name, w, b, tie in _heads(c, sd["fc.weight"], sd["fc.bias"], winner):
        with torch.no_grad():
            m.fc.weight.copy_(w)
            m.fc.bias.copy_(b)
        ref = ctx64 @ w.double().t() + b.double()
        if mode == "ragged":
            ws.get(need, xd.device).fill_(0xFF)
            lg, am = ops.model_infer(m, xd, ws, want_argmax=True, lengths=lengths)
        else:
            lg, am = m.predict(xd)
        torch.cuda.synchronize()
        lg, am = lg.cpu(), am.cpu()
        err = (lg.double() - ref).abs().max().item()
        worst = max(worst, err)
        clear = _margin(ref) >= MARGIN if c > 1 else torch.ones(5, dtype=torch.bool)
        print(f"C={c} {mode} {name}: max |logit error| {err:.2e}, argmax {am.tolist()}, {int((~clear).sum())} clips below the argmax margin"
              + (f" (smallest oracle margin {_margin(ref).min().item():.2e})" if c > 1 else ""))
        assert lg.shape == (5, c) and not lg.isnan().any()
        assert err <= tol, (name, err)
        assert torch.equal(am, lg.argmax(1)), name
        assert torch.equal(am[clear], ref.argmax(1)[clear]), name
        landed.add(int(am[0]))
        if tie is None:
            assert int((~clear).sum()) == 0, name
        else:
            p, k = tie
            assert torch.equal(lg[0, p].view(torch.int32), lg[0, k].view(torch.int32)), (name, lg[0, p].item(), lg[0, k].item())
            assert int(am[0]) == min(p, k), name
        if c == 1:
            assert am.tolist() == [0] * 5
    assert c == 1 or {0, c - 1} <= landed
    assert c <= 32 or {31, 32} <= landed
    if mode == "dense":                                   # the context vectors, read as test_model_gpu.py reads them
        dbg = {}
        lg2 = ops.model_infer(m, xd, m._ws, debug=dbg)
        torch.cuda.synchronize()
        cerr = ((dbg["ctx"].cpu().double() - ctx64).abs() / ctx64.abs().clamp(min=1.0)).max().item()
        print(f"C={c} dense: context vectors {cerr:.2e}")
        assert cerr <= CTX_TOL
        assert torch.equal(lg2.cpu(), lg)
    print(f"FIG C={c} {mode}: worst logits error {worst:.2e}")
    ops.check_status()


# ---- 3. the training step ------------------------------------------------------------------------------------------------------
def _labels(c, bsz):
    """drawn labels with C - 1 in rows 0 and 1 and class 0 in row 2; above 32 classes C - 1, 31, 32 and 0 in rows 0 to 3"""
    y = synth.synth_labels(bsz, c, seed=3001 + bsz)
    for row, label in enumerate([c - 1] + ([31, 32] if c > 32 else [c - 1]) + [0]):
        y[row] = label
    return y


def _fc_rows(m, out, c):
    """fc.weight / fc.bias gradients row by row, for every class, labelled or not"""
    gw, gb = m.fc.weight.grad.cpu().double(), m.fc.bias.grad.cpu().double()
    rw, rb = out["ref_grads"]["fc.weight"].double(), out["ref_grads"]["fc.bias"].double()
    assert gw.shape == (c, 512) and gb.shape == (c,)
    row = (gw - rw).abs().max(dim=1).values / rw.pow(2).mean(dim=1).sqrt()
    brow = (gb - rb).abs() / rb.abs()
    print(f"C={c}: fc.weight rows: worst {row.max().item():.1e} * rms (class {int(row.argmax())}), fc.bias elements: worst "
          f"{brow.max().item():.1e} * |ref| (class {int(brow.argmax())}; smallest |ref| {rb.abs().min().item():.1e})")
    assert (row <= ROW_BOUND).all() and (brow <= ROW_BOUND).all()
    return max(row.max().item(), brow.max().item())


def _case(c, bsz, t, **kw):
    out = {}
    y = _labels(c, bsz)
    assert c - 1 in y.tolist() and (c <= 32 or {31, 32} <= set(y.tolist()))
    m = _training_case(_sd(c), bsz, t, num_classes=c, labels=y, out=out, **kw)
    row = _fc_rows(m, out, c)
    dx = f"{out['dx']:.1e}" if out["dx"] is not None else "-"
    print(f"FIG C={c} ({bsz}, {t}) {kw}: loss {out['loss']:.1e} logits {out['logits']:.1e} gradient {out['grad']:.1e} norm {out['norm']:.1e} "
          f"stage {out['stage']:.1e} dfeats {dx} fc row {row:.1e}")


@pytest.mark.parametrize("c", [2, 32, 33, 63, 64])
def test_training_step_vs_oracle(c):
    _case(c, 5, 24)


@pytest.mark.parametrize("c", [33, 64])
def test_training_step_vs_oracle_with_input_gradient(c):
    _case(c, 5, 24, want_dx=True)


@pytest.mark.parametrize("c", [33, 64])
def test_training_step_vs_oracle_with_dropout(c):
    """7680 mask elements, the mask of dropout step 4 whatever ran before (the counter is put back afterwards)"""
    step = train_ops.dropout_step()
    train_ops.set_dropout_step(4)
    try:
        _case(c, 5, 24, dropout=0.5)
    finally:
        train_ops.set_dropout_step(step + 1)


@pytest.mark.parametrize("c", [33, 64])
def test_training_step_vs_oracle_17x8(c):
    """Two recurrence groups (16 + 1 clips), S = 1, a batch that is no multiple of 16: the head's grid is 17 + 2 C workgroups"""
    _case(c, 17, 8)


@pytest.mark.parametrize("c", [33, 64])
def test_frozen_statistics_input_gradient_with_supplied_dlogits(c):
    """The data-only backward under frozen statistics (sir_amd.explain's route: every BatchNorm on its running statistics, all 29
    gradient pointers NULL), where bwd_scale_kernel gives every clip a loss scale of its own from the maximum of ITS dlogits row --
    read as lane < C of one wave.  The upstream gradient is supplied: row 0 a mean cross-entropy's, row 1 has its maximum, 4.0, in
    class C - 1 >= 32 over 2^-24 * randn elsewhere (a maximum taken over lanes 0..31 alone would scale that row by 2^30 instead of
    2^5, beyond the fp16 range of the backward's operands), row 2 is a one-hot on class 32, row 3 is small throughout and row 4 has
    its maximum below class 32.  Reference: input_grad_ref.reference's supplied-dlogits entry; bound GRAD_BOUND, per clip (each on
    the rms of its own gradient: the clips are independent here and of very different magnitude) and over the batch."""
    bsz, t = 5, 24
    sd = _sd(c)
    x = cases.varied_features(bsz, t, seed=3005)
    m = CNNAudioGRU(c)
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    g = torch.Generator().manual_seed(100 + c)
    logits, leaf = explain._forward(m, x.to(DEV))
    dl = torch.empty(bsz, c)
    dl[0] = (torch.softmax(logits[0].detach().cpu(), 0) - torch.nn.functional.one_hot(torch.tensor(c - 1), c)) / bsz
    dl[1] = torch.randn(c, generator=g) * 2.0 ** -24
    dl[1, c - 1] = 4.0
    dl[2] = 0.0
    dl[2, 32] = 0.125
    dl[3] = torch.randn(c, generator=g) * 1e-5
    dl[4] = torch.randn(c, generator=g) * 1e-3
    dl[4, 7] = -2.0
    assert int(dl[1].abs().argmax()) >= 32 and int(dl[2].abs().argmax()) >= 32 and int(dl[4].abs().argmax()) < 32
    (dx,) = torch.autograd.grad(logits, leaf, grad_outputs=dl.to(DEV))
    torch.cuda.synchronize()
    zo, yo = input_grad_ref.device_forward_values(m, sd, x, bsz, t)
    _, ref_logits, ref_dx = input_grad_ref.reference(sd, x, zo, yo, bn_frozen=(True, True, True), dlogits=dl)
    lerr = (logits.detach().cpu().double() - ref_logits).abs().max().item()
    per = [input_grad_ref.ratio(dx[b], ref_dx[b]) for b in range(bsz)]
    r = input_grad_ref.ratio(dx, ref_dx)
    print(f"FIG C={c} frozen statistics, supplied dlogits: max|dx - ref| / rms(ref) = {r:.2e} over the batch, per clip "
          f"{[f'{v:.2e}' for v in per]}, logits err {lerr:.1e}")
    assert dx.shape == x.shape and torch.isfinite(dx).all()
    assert lerr < 5e-5
    assert r <= input_grad_ref.GRAD_BOUND
    assert max(per) <= input_grad_ref.GRAD_BOUND, per
    assert all(p.grad is None for p in m.parameters())
    ops.check_status()


def test_one_class_training_step_is_exactly_zero():
    """C = 1 on its own (the helper's relative figures divide by the reference's rms, which is zero here): softmax = 1, loss = 0,
    dlogits = 0, bwd_scale_pair sees a zero maximum and keeps the static scale.  Logits within 5e-5 of the oracle, the loss
    exactly 0.0, all 29 gradients and x.grad exact zeros (-0.0 accepted), the BN running statistics updated and within the
    helper's rtol 1e-4 of the oracle's."""
    bsz, t = 5, 24
    sd = _sd(1)
    x = cases.varied_features(bsz, t, seed=3005)
    m = CNNAudioGRU(1)
    m.load_state_dict(sd)
    m = m.to(DEV).train()
    m.gru.dropout = 0.0
    m.zero_grad(set_to_none=True)
    xd = x.to(DEV).requires_grad_(True)
    logits = m(xd)
    loss = train_ops.fused_cross_entropy(logits, torch.zeros(bsz, dtype=torch.int64, device=DEV))
    loss.backward()
    torch.cuda.synchronize()
    stats = {}
    with torch.no_grad():
        ref_logits = model_ref.forward(_f64(sd), x.double(), train=True, new_stats=stats)
    lerr = (logits.detach().cpu().double() - ref_logits).abs().max().item()
    grads = {n: p.grad for n, p in m.named_parameters()}
    nonzero = {n: int(torch.count_nonzero(g)) for n, g in grads.items() if g is None or int(torch.count_nonzero(g))}
    print(f"FIG C=1 (5, 24): logits err {lerr:.1e}, loss {loss.item()!r}, gradients with a non-zero element {nonzero}, "
          f"non-zero x.grad elements {int(torch.count_nonzero(xd.grad))}")
    assert logits.shape == (bsz, 1) and lerr < 5e-5
    assert loss.item() == 0.0
    assert len(grads) == 29
    for n, g in grads.items():
        assert g is not None and g.shape == dict(m.named_parameters())[n].shape, n
        assert torch.isfinite(g).all(), n
        assert torch.count_nonzero(g).item() == 0, n
    assert xd.grad.shape == xd.shape and torch.isfinite(xd.grad).all() and torch.count_nonzero(xd.grad).item() == 0
    for i in (1, 2, 3):
        bn = getattr(m, f"bn{i}")
        assert not torch.equal(bn.running_mean.cpu(), sd[f"bn{i}.running_mean"]) and int(bn.num_batches_tracked) == 1
        assert torch.allclose(bn.running_mean.cpu().double(), stats[f"bn{i}.running_mean"], rtol=1e-4, atol=1e-6)
        assert torch.allclose(bn.running_var.cpu().double(), stats[f"bn{i}.running_var"], rtol=1e-4, atol=1e-6)
    ops.check_status()


# ---- 4. a head that changes size on a live model -------------------------------------------------------------------------------
def test_head_grows_to_64_and_shrinks_to_1_on_a_live_model():
    """One module and its workspaces: inference and a training step at 31 classes, a 64-class fc (mutation_ref.swap_head), both
    again, a 1-class fc, both again.  After each swap the eval logits against the float64 oracle of the state dict the model holds
    now (running statistics as the training forwards left them) and the classifier's gradients against the oracle's; the gradient
    views of the step before must keep their values."""
    x = mr.features()
    xd = x.to(DEV)
    m = CNNAudioGRU(mr.NUM_CLASSES)
    m.load_state_dict(mr.base_state_dict())
    m = m.to(DEV)
    m.gru.dropout = 0.0
    kept = []
    for c in (mr.NUM_CLASSES, 64, 1):
        if c != mr.NUM_CLASSES:
            mr.swap_head(m, DEV, c)
        m.eval()
        sd_now = _f64(mr.cpu_state(m))
        with torch.no_grad():
            ref = model_ref.forward(sd_now, x.double())
        lg, am = m.predict(xd)
        torch.cuda.synchronize()
        err = (lg.cpu().double() - ref).abs().max().item()
        m.train()
        for p in m.parameters():
            p.grad = None
        y = synth.synth_labels(3, c, seed=3 + c)
        logits = m(xd)
        train_ops.fused_cross_entropy(logits, y.to(DEV)).backward()
        torch.cuda.synchronize()
        _, ref_grads, _, ref_logits = model_ref.loss_and_grads(sd_now, x.double(), y)
        gw, gb = m.fc.weight.grad, m.fc.bias.grad
        ew, eb = _rel(gw, ref_grads["fc.weight"])[0], _rel(gb, ref_grads["fc.bias"])[0]
        print(f"FIG head of {c} classes on the live model: eval logits err {err:.2e}, training logits err "
              f"{(logits.detach().cpu().double() - ref_logits).abs().max().item():.1e}, fc.weight gradient {ew:.1e} * rms, fc.bias {eb:.1e} * rms")
        assert lg.shape == (3, c) and err <= DENSE_TOL
        assert torch.equal(am.cpu(), lg.cpu().argmax(1))
        assert gw.shape == (c, 512) and gb.shape == (c,)
        assert all(p.grad is not None and p.grad.shape == p.shape and torch.isfinite(p.grad).all() for p in m.parameters())
        assert ew < 2e-3 and eb < 2e-3                    # (C = 1: the reference is zero, rms = 0, and so must the device be)
        for grads, values in kept:
            for g, v in zip(grads, values):
                assert torch.equal(g, v), "an earlier step's gradient was overwritten through a stale view"
        grads = [p.grad for p in m.parameters()]
        kept.append((grads, [g.clone() for g in grads]))
        ops.check_status()


# ---- 5. outside the range ----------------------------------------------------------------------------------------------------
def test_sixty_five_classes_are_refused_and_leave_nothing_behind():
    x = cases.varied_features(5, 24, seed=3005).to(DEV)
    m64 = CNNAudioGRU(64)
    m64.load_state_dict(_sd(64))
    m64 = m64.to(DEV).train()
    m64.gru.dropout = 0.0
    m65 = CNNAudioGRU(65)
    m65.load_state_dict(synth.synth_state_dict(65, seed=0))
    m65 = m65.to(DEV).eval()
    tl = m64(x).detach().clone()
    m64.load_state_dict(_sd(64))                          # (the running statistics the training forward moved)
    m64.eval()
    lg, am = m64.predict(x)
    lg, am = lg.clone(), am.clone()
    lengths = torch.tensor(LENGTHS, dtype=torch.int32, device=DEV)
    calls = {"predict": lambda: m65.predict(x),
             "predict on the 64-class model's workspace": lambda: ops.model_infer(m65, x, m64._ws, want_argmax=True),
             "ragged": lambda: m65.predict(x, lengths=lengths),
             "training forward": lambda: m65.train()(x),
             "loss": lambda: train_ops.fused_cross_entropy(torch.zeros(5, 65, device=DEV), torch.zeros(5, dtype=torch.int64, device=DEV))}
    for name, call in calls.items():
        with pytest.raises(_native.SirError, match="num_classes") as e:
            call()
        print(f"{name}: {e.value}")
        m65.eval()
        ops.check_status()
    lg2, am2 = m64.predict(x)
    assert torch.equal(lg2, lg) and torch.equal(am2, am)
    m64.train()
    assert torch.equal(m64(x).detach(), tl)
    ops.check_status()
