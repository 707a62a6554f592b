"""More than one live node of the differentiable step per model: programs whose forwards and backwards interleave.

Every other training-path test runs forward, backward, forward, backward.  The step is an ordinary ``torch.autograd.Function``,
so users also write ``(ce(model(x1), y1) + ce(model(x2), y2)).backward()``, or probe the model (``explain``, the adversary's
crafting pass, ``predict``) between a forward and its backward.  What a node needs between its forward and its backward -- the
workspace with its activations, the flat gradient buffer, unchanged inputs -- is what these tests are about.

Reference: the same steps run ONE AT A TIME on a fresh copy of the model (``_run_lone``); the rest of the suite pins those lone
steps to the float64 oracle.  Same kernels on the same inputs give the same bits, and one fp32 add commutes, so the parameter
gradients of a two-node program must be ``torch.equal`` to ``gA + gB`` of the lone steps; three nodes are compared with
``torch.allclose(rtol=1e-6, atol=1e-9)``, the bound of ``test_gradient_hand_over_matches_autograd_accumulation``.  The order
of the two adds is autograd's, and where the three terms cancel two orders differ by up to 6e-7 * rms, more than that bound:
the program must meet it against the lone gradients added in SOME order, the same one for every parameter.  ``x.grad`` and
the BatchNorm running statistics (two momentum updates in forward order) are compared bit for bit as well.  One anchor to
the oracle itself: the two-node same-shape case compares the GRU / attention / fc gradients with the sum of two
``model_ref.loss_and_grads`` calls at the project's bound for those tensors, ``< 2e-3 * rms`` (``test_train_gpu.py``); conv /
BN tensors need the device-value overrides of one workspace and are covered by the bit identity.

Shapes: (3, 24), (2, 16) and (5, 40) frames -- the smallest that go through every kernel; the second fits in the first's
workspace, the third makes it regrow.  31 classes, ``cases.varied_features`` inputs, dropout off except in one case.
"""
import functools
import itertools
import operator
from typing import NamedTuple

import pytest
import torch

import cases
from oracle import model_ref
from sir_amd import explain, finetune, ops, synth, train_ops
from sir_amd.models.models import CNNAudioGRU
from sir_amd.optim import FusedAdam
from sir_amd.prototypes import ProxyHead
from train_step_ref import _rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
NCLS = 31
ce = train_ops.fused_cross_entropy


class Node(NamedTuple):
    """One forward of a program: its batch, the loss put on it and what is done to the model just before it."""
    bsz: int
    t: int
    seed: int
    kind: str = "ce"             # "ce": cross-entropy on model(x); "emb": a loss on the embedding alone; "metric": MetricLoss
    x_grad: bool = False
    lengths: tuple = None        # the ragged step (needs frozen BatchNorm statistics)
    setup: str = None            # key of SETUPS, applied to the model before this forward
    key: int = None              # dropout step counter value this forward draws


A = Node(3, 24, 11, x_grad=True)
B = Node(3, 24, 21)
SMALL = Node(2, 16, 31, x_grad=True)
LARGE = Node(5, 40, 41, x_grad=True)

SETUPS = {"freeze_fc_bias": lambda m: m.fc.bias.requires_grad_(False),
          "thaw_fc_bias": lambda m: m.fc.bias.requires_grad_(True)}
PREPARE = {None: lambda m: None, "bn_stats": lambda m: finetune.freeze(m, {"bn_stats"})}


@functools.lru_cache(maxsize=None)
def _sd():
    return synth.synth_state_dict(NCLS, seed=0)


@functools.lru_cache(maxsize=None)
def _data(bsz, t, seed):
    return cases.varied_features(bsz, t, seed=seed), synth.synth_labels(bsz, NCLS, seed=seed + 1)


@functools.lru_cache(maxsize=None)
def _emb_weights(bsz, seed):
    return torch.randn(bsz, 512, generator=torch.Generator().manual_seed(seed + 2)) / bsz


def _fresh(dropout=0.0, prepare=None):
    m = CNNAudioGRU(NCLS)
    m.load_state_dict(_sd())
    m = m.to(DEV).train()
    m.gru.dropout = dropout
    PREPARE[prepare](m)
    return m, ProxyHead(NCLS, seed=3).to(DEV)


def _forward(m, head, nd):
    """``(loss, x on the device, the dropout key the forward drew)``"""
    x, y = _data(nd.bsz, nd.t, nd.seed)
    xd = x.to(DEV).requires_grad_(nd.x_grad)
    if nd.setup is not None:
        SETUPS[nd.setup](m)
    if nd.key is not None:
        train_ops.set_dropout_step(nd.key)
    kw = {"lengths": list(nd.lengths)} if nd.lengths is not None else {}
    if nd.kind == "ce":
        loss = ce(m(xd, **kw), y.to(DEV))
    elif nd.kind == "emb":
        _, emb = m.forward_with_embedding(xd, **kw)
        loss = (emb * _emb_weights(nd.bsz, nd.seed).to(DEV)).sum()
    else:
        loss = train_ops.MetricLoss(head, weight=0.5).loss(m, xd, y.to(DEV), ce)
    return loss, xd, getattr(m, "_sir_last_dropout", None)


def _params(m, head):
    return dict(m.named_parameters(), proxies=head.proxies)


def _grads(m, head):
    return {n: p.grad.clone() if p.grad is not None else None for n, p in _params(m, head).items()}


def _bn_state(m):
    return {f"bn{i}.{k}": getattr(getattr(m, f"bn{i}"), k).clone()
            for i in (1, 2, 3) for k in ("running_mean", "running_var", "num_batches_tracked")}


class Lone(NamedTuple):
    grads: dict
    xgrad: torch.Tensor
    drop: tuple


def _run_lone(nodes, dropout=0.0, prepare=None):
    """The reference: the steps of ``nodes`` one at a time (forward, backward, ``zero_grad(set_to_none=True)``) on a fresh model.
    Returns the model, the head, one ``Lone`` per step and the BatchNorm buffers after the last."""
    m, head = _fresh(dropout, prepare)
    out = []
    for nd in nodes:
        m.zero_grad(set_to_none=True)
        head.zero_grad(set_to_none=True)
        loss, xd, drop = _forward(m, head, nd)
        loss.backward()
        out.append(Lone(_grads(m, head), xd.grad.clone() if nd.x_grad else None, drop))
    torch.cuda.synchronize()
    return m, head, out, _bn_state(m)


@functools.lru_cache(maxsize=None)
def _lone(nodes, dropout=0.0, prepare=None):
    """``_run_lone`` computed once per program and shared; nothing it returns is changed by a test."""
    return _run_lone(nodes, dropout, prepare)[2:]


def _interleaved(nodes, order=None, dropout=0.0, prepare=None, before=None):
    """All forwards of ``nodes`` on one fresh model, then one backward pass over the sum of the losses (``order is None``) or
    one backward per loss in ``order``, with no ``zero_grad`` in between."""
    m, head = _fresh(dropout, prepare)
    if before is not None:
        before(m, head)
    fw = [_forward(m, head, nd) for nd in nodes]
    if order is None:
        functools.reduce(operator.add, [f[0] for f in fw]).backward()
    else:
        for i in order:
            fw[i][0].backward()
    torch.cuda.synchronize()
    return m, head, fw


def _sum(parts):
    """The lone steps' gradients added up in fp32, left to right (the order matters from three terms on)."""
    out = {}
    for name in parts[0].grads:
        gs = [p.grads[name] for p in parts if p.grads[name] is not None]
        out[name] = functools.reduce(operator.add, gs) if gs else None
    return out


def _misses(got, want, exact):
    """``{parameter: what is wrong}`` of the gradients in ``got`` against ``want``: bit for bit, or within the three-node bound."""
    out = {}
    for n, w in want.items():
        g = got[n].grad
        if (g is None) != (w is None):
            out[n] = "has a gradient" if w is None else "has no gradient"
        elif w is not None and not (torch.equal(g, w) if exact else torch.allclose(g, w, rtol=1e-6, atol=1e-9)):
            out[n] = f"{_rel(g, w)[0]:.2e} * rms"
    return out


def _check(label, m, head, fw, nodes, parts, bn, exact=True):
    """Parameter gradients == the sum of the lone steps' (``parts``, one per node), each wanted ``x.grad`` and dropout key ==
    its lone step's, BatchNorm buffers == ``bn``; the worst gradient error is printed before anything is asserted.  Not
    ``exact`` (three nodes): within the bound of the sum taken in one of its orders -- which one is the autograd engine's choice."""
    got = _params(m, head)
    want = _sum(parts)
    errs = {n: _rel(got[n].grad, w)[0] for n, w in want.items() if w is not None and got[n].grad is not None}
    worst = max(errs, key=errs.get)
    print(f"{label}: worst parameter gradient error {errs[worst]:.2e} * rms ({worst})")
    orders = [parts] if exact else list(itertools.permutations(parts))
    misses = [_misses(got, _sum(order), exact) for order in orders]
    assert any(not mi for mi in misses), (label, min(misses, key=len))
    for (_, xd, drop), nd, part in zip(fw, nodes, parts):
        if nd.x_grad:
            assert xd.grad is not None and xd.grad.shape == xd.shape
            assert torch.equal(xd.grad, part.xgrad), (nd, _rel(xd.grad, part.xgrad)[0])
        if nd.key is not None:
            assert drop == part.drop and drop[1] > 0.0, (nd, drop, part.drop)
    for k, v in _bn_state(m).items():
        assert torch.equal(v, bn[k]), k
    ops.check_status()


# ---- 1. two nodes, one backward pass, same shape ---------------------------------------------------------------------------
def test_two_nodes_one_backward_hand_over_path_and_oracle_anchor():
    """``p.grad is None`` everywhere: the path on which a lone node hands its views over.  Also the anchor to the oracle."""
    parts, bn = _lone((A, B))
    m, head, fw = _interleaved((A, B))
    _check("two nodes, hand-over path", m, head, fw, (A, B), parts, bn)
    ref = [model_ref.loss_and_grads(_sd(), *_data(nd.bsz, nd.t, nd.seed))[1] for nd in (A, B)]
    for name, p in m.named_parameters():
        if name.startswith(("conv", "bn")):
            continue
        r = ref[0][name] + ref[1][name]
        if r.abs().max() <= 1e-7:                    # (attention.bias: zero in exact arithmetic)
            continue
        e = _rel(p.grad, r)[0]
        assert e < 2e-3, (name, e)


def _leave_zeroed_grads(m, head):
    """An earlier step, then ``zero_grad(set_to_none=False)``: every ``.grad`` is a zeroed VIEW of the flat gradient buffer."""
    loss, _, _ = _forward(m, head, A)
    loss.backward()
    m.zero_grad(set_to_none=False)
    flat = m._sir_train["grads"].flat
    assert all(flat.data_ptr() <= p.grad.data_ptr() < flat.data_ptr() + 4 * flat.numel() for p in m.parameters())


def _hook_one_parameter(m, head):
    m.gru.weight_hh_l1.register_hook(lambda g: None)


@pytest.mark.parametrize("form", ["leftover_grad", "hook"])
def test_two_nodes_one_backward_autograd_path(form):
    """A ``.grad`` left from an earlier step, or a gradient hook on one parameter: the node returns its gradients through
    autograd, which holds the first node's result by reference until the second has run."""
    if form == "leftover_grad":
        parts, bn = _lone((A, A, B))                 # (the earlier step moved the running statistics once more)
        parts = parts[1:]
        m, head, fw = _interleaved((A, B), before=_leave_zeroed_grads)
    else:
        parts, bn = _lone((A, B))
        m, head, fw = _interleaved((A, B), before=_hook_one_parameter)
    _check(f"two nodes, autograd path ({form})", m, head, fw, (A, B), parts, bn)


# ---- 2. two nodes of different shapes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("nodes", [(LARGE, A), (A, LARGE)], ids=["second_fits_in_first", "buffer_regrows"])
@pytest.mark.parametrize("form", ["hand_over", "hook"])
def test_two_nodes_of_different_shapes(nodes, form):
    """(5, 40) then (3, 24): the second forward fits in the first's workspace.  (3, 24) then (5, 40): it needs a larger one --
    with a hook, this is the flat-buffer alias with nothing else in the way."""
    parts, bn = _lone(nodes)
    m, head, fw = _interleaved(nodes, before=_hook_one_parameter if form == "hook" else None)
    _check(f"two shapes {nodes[0][:2]} {nodes[1][:2]} ({form})", m, head, fw, nodes, parts, bn)


# ---- 3. separate backwards in both orders ----------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [(0, 1), (1, 0)], ids=["bwd_a_bwd_b", "bwd_b_bwd_a"])
def test_two_nodes_separate_backwards(order):
    parts, bn = _lone((A, B))
    m, head, fw = _interleaved((A, B), order=order)
    _check(f"separate backwards {order}", m, head, fw, (A, B), parts, bn)


# ---- 4. three live nodes ---------------------------------------------------------------------------------------------------
def test_three_nodes_one_backward():
    nodes = (A, SMALL, LARGE)
    parts, bn = _lone(nodes)
    m, head, fw = _interleaved(nodes)
    _check("three nodes", m, head, fw, nodes, parts, bn, exact=False)


def test_two_nodes_with_dropout_draw_the_keys_of_their_lone_steps():
    """Dropout on: each node's backward must rebuild the mask of ITS forward's key (101 / 202), not the latest one."""
    a, b = A._replace(key=101), B._replace(key=202)
    parts, bn = _lone((a, b), dropout=0.5)
    assert parts[0].drop[0] != parts[1].drop[0]
    m, head, fw = _interleaved((a, b), dropout=0.5)
    _check("two nodes, dropout 0.5", m, head, fw, (a, b), parts, bn)


# ---- 5. a call that uses the training workspace but joins no graph, between a forward and its backward ---------------------
def _probe_input_gradient(m):
    logits, dx = explain.input_gradient(m, _data(2, 16, 31)[0].to(DEV))
    return logits, dx


def _probe_craft(m):
    x, y = _data(2, 16, 31)
    logits, leaf = train_ops.forward_craft(m, x.to(DEV))
    (g,) = torch.autograd.grad(ce(logits, y.to(DEV)), leaf)
    return logits.detach(), g


def _probe_predict(m):
    m.eval()
    out = m.predict(_data(2, 16, 31)[0].to(DEV))
    m.train()
    return out


@pytest.mark.parametrize("probe", [_probe_input_gradient, _probe_craft, _probe_predict], ids=["input_gradient", "forward_craft", "predict"])
def test_probe_between_forward_and_backward(probe):
    """fwd A, probe on a (2, 16) batch (it fits in A's workspace), bwd A.  The reference probe runs on the lone model after its
    step A: same weights, same running statistics."""
    m_ref, _, parts, bn = _run_lone((A,))
    want = probe(m_ref)
    assert all(torch.equal(v, b) for v, b in zip(_bn_state(m_ref).values(), bn.values()))     # a probe leaves the module alone
    m, head = _fresh()
    loss, xd, drop = _forward(m, head, A)
    got = probe(m)
    loss.backward()
    torch.cuda.synchronize()
    _check(f"probe {probe.__name__}", m, head, [(loss, xd, drop)], (A,), parts, bn)
    for g, w in zip(got, want):
        assert torch.equal(g, w), probe.__name__


# ---- 6. forward_with_embedding nodes ---------------------------------------------------------------------------------------
def test_embedding_only_node_beside_a_cross_entropy_node():
    nodes = (A._replace(kind="emb"), B)
    parts, bn = _lone(nodes)
    m, head, fw = _interleaved(nodes)
    _check("embedding-only node + CE node", m, head, fw, nodes, parts, bn)


def test_two_metric_loss_nodes():
    """Two nodes carrying ``ProxyHead``'s loss as ``MetricLoss`` builds it; the proxies' own gradient is summed as well."""
    nodes = (A._replace(kind="metric"), B._replace(kind="metric"))
    parts, bn = _lone(nodes)
    assert parts[0].grads["proxies"] is not None
    m, head, fw = _interleaved(nodes)
    _check("two MetricLoss nodes", m, head, fw, nodes, parts, bn)


# ---- 7. two live ragged nodes ----------------------------------------------------------------------------------------------
def test_two_ragged_nodes_with_different_lengths():
    a = A._replace(lengths=(24, 9, 17))
    b = B._replace(lengths=(8, 24, 13), x_grad=True)
    parts, bn = _lone((a, b), prepare="bn_stats")
    m, head, fw = _interleaved((a, b), prepare="bn_stats")
    _check("two ragged nodes", m, head, fw, (a, b), parts, bn)
    for (_, xd, _), nd in zip(fw, (a, b)):
        for row, n in enumerate(nd.lengths):
            assert (xd.grad[row, :, n:] == 0).all() and (xd.grad[row, :, :n] != 0).any(), (nd, row)
    assert all(int(getattr(m, f"bn{i}").num_batches_tracked) == 0 for i in (1, 2, 3))


# ---- 8. frozen layers ------------------------------------------------------------------------------------------------------
def test_each_node_gets_the_gradients_its_own_forward_saw():
    """Node A is created while ``fc.bias`` is frozen, node B after it is trainable again: ``fc.bias.grad`` is B's alone."""
    nodes = (A._replace(setup="freeze_fc_bias"), B._replace(setup="thaw_fc_bias"))
    parts, bn = _lone(nodes)
    assert parts[0].grads["fc.bias"] is None and parts[1].grads["fc.bias"] is not None
    m, head, fw = _interleaved(nodes)
    _check("frozen fc.bias in one node", m, head, fw, nodes, parts, bn)
    assert torch.equal(m.fc.bias.grad, parts[1].grads["fc.bias"])


# ---- 9. retain_graph -------------------------------------------------------------------------------------------------------
def test_backward_twice_with_nothing_in_between_keeps_working():
    """``test_operand_range_gpu.py`` runs many backwards through one retained node."""
    parts, bn = _lone((A,))
    m, head = _fresh()
    loss, xd, drop = _forward(m, head, A)
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        xd.grad = None
        loss.backward(retain_graph=True)
        _check("retained graph, backward again", m, head, [(loss, xd, drop)], (A,), parts, bn)
    loss.backward()                                  # no zero_grad: accumulates
    for n, p in m.named_parameters():
        assert torch.allclose(p.grad, 2.0 * parts[0].grads[n], rtol=1e-6, atol=1e-9), n


def test_backward_again_after_another_forward_raises():
    """bwd A, fwd B, bwd A again: A's workspace went back to the model at the end of its first backward and B's forward took it.
    Documented (``CNNAudioGRU.forward``): ``RuntimeError``.  B's own step is unharmed."""
    parts, bn = _lone((A, B))
    m, head = _fresh()
    loss_a, _, _ = _forward(m, head, A)
    loss_a.backward(retain_graph=True)
    loss_b, xd, drop = _forward(m, head, B)
    with pytest.raises(RuntimeError, match="retain_graph.*backward again after another forward on this model"):
        loss_a.backward()
    m.zero_grad(set_to_none=True)
    loss_b.backward()
    _check("B after A's refused second backward", m, head, [(loss_b, xd, drop)], (B,), parts[1:], bn)


# ---- 10. stale inputs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("modify", [True, False], ids=["x_changed_in_place", "control"])
def test_input_changed_in_place_before_backward_raises(modify):
    parts, bn = _lone((B,))
    m, head = _fresh()
    x, y = _data(B.bsz, B.t, B.seed)
    xd = x.to(DEV)
    loss = ce(m(xd), y.to(DEV))
    if modify:
        xd.add_(1)
        with pytest.raises(RuntimeError, match="modified by an inplace operation"):
            loss.backward()
        assert all(p.grad is None for p in m.parameters())
    else:
        loss.backward()
        _check("control: x untouched", m, head, [(loss, xd, None)], (B,), parts, bn)
    ops.check_status()


@pytest.mark.parametrize("modify", ["fused_adam", "torch_in_place", None])
def test_weights_changed_before_backward_raises(modify):
    """``FusedAdam.step()`` writes behind torch's version counters; an in-place torch update moves them.  Either one between a
    node's forward and its backward raises; the same program without it does not."""
    parts, bn = _lone((A, B))
    m, head = _fresh()
    opt = FusedAdam(m.parameters(), lr=1e-3)
    _forward(m, head, A)[0].backward()               # leftover gradients for the optimizer
    loss, xd, drop = _forward(m, head, B)
    if modify is None:
        m.zero_grad(set_to_none=True)
        loss.backward()
        _check("control: weights untouched", m, head, [(loss, xd, drop)], (B,), parts[1:], bn)
        return
    if modify == "fused_adam":
        opt.step()
    else:
        with torch.no_grad():
            m.fc.bias.mul_(0.5)
    m.zero_grad(set_to_none=True)
    with pytest.raises(RuntimeError, match="changed in place between this node's forward and its backward"):
        loss.backward()
    assert all(p.grad is None for p in m.parameters())
    # the refused node gave its workspace back: the next step runs on the module's own buffer
    again, _, _ = _forward(m, head, B)               # (the refused node's graph is still alive)
    pool = m._sir_train["pool"]
    assert pool.primary_held and len(pool.live) == 1 and not pool.free
    again.backward()
    ops.check_status()


@pytest.mark.parametrize("entry", ["forward_craft", "explain"])
@pytest.mark.parametrize("modify", ["x", "fused_adam", None])
def test_crafting_pass_and_explain_check_stale_inputs(entry, modify):
    """The nodes without a step (``forward_craft``; ``explain._forward``, what every function of ``explain`` runs) record and
    check as the training node does: ``x`` or a weight changed between the forward and ``autograd.grad`` raises; left alone,
    the gradient is that of the same call made again."""
    forward = train_ops.forward_craft if entry == "forward_craft" else explain._forward
    m, head = _fresh()
    opt = FusedAdam(m.parameters(), lr=1e-3)
    _forward(m, head, A)[0].backward()               # leftover gradients for the optimizer
    x, y = _data(2, 16, 31)
    x, y = x.to(DEV), y.to(DEV)
    logits, leaf = forward(m, x)
    loss = ce(logits, y)
    if modify == "x":
        x.add_(1)                                    # (the leaf is x detached: same storage, same version counter)
        with pytest.raises(RuntimeError, match="modified by an inplace operation"):
            torch.autograd.grad(loss, leaf)
    elif modify == "fused_adam":
        opt.step()
        with pytest.raises(RuntimeError, match="changed in place between this node's forward and its backward"):
            torch.autograd.grad(loss, leaf)
    else:
        (g,) = torch.autograd.grad(loss, leaf)
        logits2, leaf2 = forward(m, x)
        (g2,) = torch.autograd.grad(ce(logits2, y), leaf2)
        assert torch.equal(logits, logits2) and torch.equal(g, g2) and bool(g.abs().max() > 0)
    pool = m._sir_train["pool"]
    assert not pool.primary_held and len(pool.live) == 0       # refused or not, the node gave its workspace back
    ops.check_status()


# ---- 11. the ordinary loop pays nothing ------------------------------------------------------------------------------------
def _assert_handed_over(m, want):
    flat = m._sir_train["grads"].flat
    for n, p in m.named_parameters():
        assert torch.equal(p.grad, want[n]), n
        assert flat.data_ptr() <= p.grad.data_ptr() < flat.data_ptr() + 4 * flat.numel(), n     # handed over, not cloned


def test_plain_loop_keeps_one_workspace_and_the_hand_over():
    parts, _ = _lone((A,))
    m, head = _fresh()
    seen = set()
    for _ in range(4):
        loss, _, _ = _forward(m, head, A)            # (the previous loss is still alive here, as in train_epoch)
        loss.backward()
        ws = m._sir_train["ws"]
        seen.add((ws.buf.data_ptr(), ws.generation))
        _assert_handed_over(m, parts[0].grads)
        m.zero_grad(set_to_none=True)
    assert len(seen) == 1, seen
    # an interleaved step, then the plain loop again: still the views of the flat buffer, still the one workspace
    la, lb = _forward(m, head, A)[0], _forward(m, head, B)[0]
    (la + lb).backward()
    m.zero_grad(set_to_none=True)
    loss, _, _ = _forward(m, head, A)
    loss.backward()
    ws = m._sir_train["ws"]
    assert (ws.buf.data_ptr(), ws.generation) in seen
    _assert_handed_over(m, parts[0].grads)
    ops.check_status()


def test_interleaved_step_leaks_no_workspace():
    m, head = _fresh()

    def plain():
        _forward(m, head, A)[0].backward()
        m.zero_grad(set_to_none=True)

    def interleaved():
        la, lb, lc = (_forward(m, head, nd)[0] for nd in (A, B, A))
        assert len(m._sir_train["pool"].live) == 3   # three nodes, each holding a workspace of its own
        (la + lb + lc).backward()
        m.zero_grad(set_to_none=True)

    plain()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    interleaved()                                    # (its losses die with the call)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == base
    plain()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == base
    ops.check_status()
