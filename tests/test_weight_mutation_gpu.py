"""Every way a model's weights can change between two calls on the SAME model object.

The model keeps two things between calls: the ``sir_model_weights`` pointer struct (``ops.cached_weights``) and, inside the
workspace, the layouts ``sir_model_infer`` prepares from some of the tensors (folded BatchNorm, Winograd planes of conv2 / conv3,
f16 splits of ``weight_ih``, fragments of ``weight_hh``), reused while ``ops.weights_version`` is unchanged.  A stale struct or a
stale layout gives plausible logits of the OLD weights, which no fresh-model parity test can see.

Every case here is: call, change the weights, call again at the same (B, T), compare with ``oracle.model_ref.forward`` on the state
dict the model now holds -- ``|logits - oracle| < 2e-5`` (``mutation_ref.TOL``) -- after asserting that the ORACLE's logits moved by
at least 1e-3 (``mutation_ref.FLOOR``, 50 x the bound: the old result cannot pass).  Model ``synth_state_dict(31, seed=0)``, input
``synth_features(3, 64, seed=21)``; the ragged calls use lengths [64, 40, 9] and the oracle row by row.  No case asserts that
a stale result IS stale; every case ends in ``ops.check_status()``.

The state dict has 38 entries: 35 float tensors (29 parameters, 6 running statistics) and the three integer
``num_batches_tracked``.  ``attention.bias`` cannot move the logits, so 34 tensors are mutated one at a time."""
import copy
import ctypes as C

import pytest
import torch

import mutation_ref as mr
from oracle import model_ref
from sir_amd import _native, ops, synth, train_ops
from sir_amd.featurizer import get_featurizer
from sir_amd.models.models import CNNAudioGRU
from sir_amd.optim import FusedAdam
from train_step_ref import _rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS = mr.float_keys(mr.base_state_dict())


@pytest.fixture(autouse=True)
def _status_is_clean():
    yield
    ops.check_status()


def _oracle(sd, x, lengths=None):
    with torch.no_grad():
        if lengths is None:
            return model_ref.forward(sd, x)
        return torch.cat([model_ref.forward(sd, x[b:b + 1, :, :f]) for b, f in enumerate(lengths)])


@pytest.fixture(scope="module")
def base():
    """the un-mutated state dict, the input and the oracle's logits for the padded and the ragged call (computed once)"""
    sd, x = mr.base_state_dict(), mr.features()
    return {"sd": sd, "x": x, "ref": _oracle(sd, x), "ref_ragged": _oracle(sd, x, mr.LENGTHS)}


_mutated_refs = {}


def _mutated_ref(base, key):
    """(state dict with ``key`` mutated, oracle padded, oracle ragged), computed once per tensor and shared by its cases"""
    if key not in _mutated_refs:
        sd = dict(base["sd"])
        sd[key] = mr.mutated(key, sd[key])
        _mutated_refs[key] = (sd, _oracle(sd, base["x"]), _oracle(sd, base["x"], mr.LENGTHS))
    return _mutated_refs[key]


def _model(sd, num_classes=mr.NUM_CLASSES):
    m = CNNAudioGRU(num_classes)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def _assert_close(got, ref, what):
    err = (got.detach().cpu() - ref).abs().max().item()
    print(f"{what}: max |logits - oracle| {err:.3e}")
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert err < mr.TOL, (what, err)


def _assert_moved(ref, before, what, floor=mr.FLOOR):
    moved = (ref - before).abs().max().item() if ref.shape == before.shape else float("inf")
    print(f"{what}: the oracle moved by {moved:.3e}")
    assert moved >= floor, (what, moved)


def _check_now(m, x, before, what, lengths=None, floor=mr.FLOOR):
    """the model's next call against the oracle of the state dict it holds NOW, which must differ from ``before``"""
    ref = _oracle(mr.cpu_state(m), x, lengths)
    _assert_moved(ref, before, what, floor)
    _assert_close(m(x.to(DEV), lengths=lengths), ref, what)
    return ref


# ---- a. one tensor at a time ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ragged", [False, True], ids=["padded", "ragged"])
@pytest.mark.parametrize("key", KEYS)
def test_in_place_update_of_one_tensor(base, key, ragged):
    """``with torch.no_grad(): t.add_(...)``: torch's version counter moves, the fingerprint must follow it for every tensor
    -- the prepared group and the group the kernels read directly alike."""
    lengths = mr.LENGTHS if ragged else None
    before = base["ref_ragged" if ragged else "ref"]
    sd2, ref_padded, ref_ragged = _mutated_ref(base, key)
    ref = ref_ragged if ragged else ref_padded
    m = _model(base["sd"])
    x = base["x"].to(DEV)
    _assert_close(m(x, lengths=lengths), before, f"{key} before")
    with torch.no_grad():
        mr.mutate_(mr.tensor_of(m, key), key, base["sd"][key])
    assert torch.equal(mr.tensor_of(m, key).detach().cpu(), sd2[key])          # the oracle and the device hold the same bits
    _assert_moved(ref, before, key)
    _assert_close(m(x, lengths=lengths), ref, f"{key} after")


@pytest.mark.parametrize("key", KEYS)
def test_data_update_of_one_tensor_with_weights_changed(base, key):
    """``t.data.add_(...)`` moves no version counter; ``model.weights_changed()`` is the documented call that follows it."""
    sd2, ref, _ = _mutated_ref(base, key)
    m = _model(base["sd"])
    x = base["x"].to(DEV)
    _assert_close(m(x), base["ref"], f"{key} before")
    mr.mutate_(mr.tensor_of(m, key).data, key, base["sd"][key])
    m.weights_changed()
    assert torch.equal(mr.tensor_of(m, key).detach().cpu(), sd2[key])
    _assert_moved(ref, base["ref"], key)
    _assert_close(m(x), ref, f"{key} after")


# ---- b. identity changes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [r for r in mr.ROUTES if r != "head_swap"])
def test_replaced_tensors(base, route):
    """Routes that give the module another tensor (another storage address) under the same name: the pointer struct must be
    rebuilt, and the layouts prepared from the old tensor must not be reused."""
    m = _model(base["sd"])
    x = base["x"]
    _assert_close(m(x.to(DEV)), base["ref"], f"{route} before")
    _assert_close(m(x.to(DEV), lengths=mr.LENGTHS), base["ref_ragged"], f"{route} before, ragged")
    mr.ROUTES[route](m, DEV)
    _check_now(m, x, base["ref"], route)
    _check_now(m, x, base["ref_ragged"], route + ", ragged", lengths=mr.LENGTHS)


def test_head_swap_to_six_classes(base):
    """``model.fc = nn.Linear(512, 6)``: logits [3, 6] of the new head; ``predict`` and ``classify`` agree with the oracle's argmax
    (its top-2 margins on these rows are >= 6e-3, 300 x the bound)."""
    m = _model(base["sd"])
    x = base["x"]
    _assert_close(m(x.to(DEV)), base["ref"], "31 classes")
    mr.swap_head(m, DEV)
    ref = _check_now(m, x, base["ref"], "head swap")
    assert ref.shape == (3, mr.NEW_CLASSES)
    top2 = ref.topk(2).values
    assert (top2[:, 0] - top2[:, 1]).min() >= 1e-3
    logits, amax = m.predict(x.to(DEV))
    _assert_close(logits, ref, "predict")
    assert torch.equal(amax.cpu(), ref.argmax(1))
    logits, idx, prob = m.classify(x.to(DEV), k=3)
    _assert_close(logits, ref, "classify")
    assert torch.equal(idx[:, 0].cpu().long(), ref.argmax(1))
    assert (prob.cpu() - torch.softmax(ref, 1).topk(3).values).abs().max() < 1e-5
    _assert_close(m(x.to(DEV), lengths=mr.LENGTHS), _oracle(mr.cpu_state(m), x, mr.LENGTHS), "ragged")


class _LibSpy:
    """the loaded library with the names of the entry points that were looked up"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        self.calls.append(name)
        return getattr(self._lib, name)


def test_half_is_refused_and_float_recovers(base, monkeypatch):
    """``model.half()``: ``SirError`` before anything is launched (the only library call is the host-side workspace size);
    ``model.float()`` afterwards runs on the fp16-rounded values (the oracle moves by 1.6e-4 on them: the floor here is 1e-4)."""
    m = _model(base["sd"])
    x = base["x"]
    _assert_close(m(x.to(DEV)), base["ref"], "float32")
    m.half()
    spy = _LibSpy(_native.lib())
    monkeypatch.setattr(_native, "lib", lambda: spy)
    for call in (lambda: m(x.to(DEV)), lambda: m(x.to(DEV), lengths=mr.LENGTHS), lambda: m.predict(x.to(DEV))):
        with pytest.raises(_native.SirError, match="float32"):
            call()
    assert set(spy.calls) <= {"sir_model_workspace_bytes"}, spy.calls
    monkeypatch.undo()
    m.float()
    _check_now(m, x, base["ref"], "half -> float", floor=1e-4)


# ---- c. copies --------------------------------------------------------------------------------------------------------------
def _struct_pointers(m):
    w, _ = ops.cached_weights(m)
    out = [w.attn_w, w.attn_b, w.fc_w, w.fc_b]
    for field in ("conv_w", "bn_w", "bn_b", "bn_mean", "bn_var", "gru_w_ih", "gru_w_hh", "gru_b_ih", "gru_b_hh"):
        out += list(getattr(w, field))
    return w, out


@pytest.mark.parametrize("when", ["before_first_forward", "after_one_forward"])
def test_deepcopy_is_independent(base, when):
    m = _model(base["sd"])
    x = base["x"]
    if when == "after_one_forward":
        _assert_close(m(x.to(DEV)), base["ref"], "original, first call")
    c = copy.deepcopy(m)
    a, b = m(x.to(DEV)), c(x.to(DEV))
    _assert_close(a, base["ref"], "original")
    assert torch.equal(a, b)                                                    # same weights, same kernels: bit for bit
    assert c._sir_token != m._sir_token
    assert c._ws is not m._ws and c._ws.buf.data_ptr() != m._ws.buf.data_ptr()
    (wm, pm), (wc, pc) = _struct_pointers(m), _struct_pointers(c)
    assert wm is not wc and not set(pm) & set(pc)
    assert pc[2] == c.fc.weight.data_ptr() and pm[2] == m.fc.weight.data_ptr()
    # the copy changes: the original keeps its own oracle, bit for bit
    with torch.no_grad():
        mr.mutate_(c.conv3.weight, "conv3.weight", base["sd"]["conv3.weight"])
    ref_c = _check_now(c, x, base["ref"], "copy after its own update")
    assert torch.equal(m(x.to(DEV)), a)
    # then the original changes too
    with torch.no_grad():
        mr.mutate_(m.gru.weight_hh_l1, "gru.weight_hh_l1", base["sd"]["gru.weight_hh_l1"])
    _check_now(m, x, base["ref"], "original after its own update")
    _assert_close(c(x.to(DEV)), ref_c, "copy after the original's update")
    _check_now(m, x, base["ref_ragged"], "original, ragged", lengths=mr.LENGTHS)
    _check_now(c, x, base["ref_ragged"], "copy, ragged", lengths=mr.LENGTHS)


# ---- d. optimizers that are not ours ----------------------------------------------------------------------------------------
def _train_backward(m, x, y):
    m.train()
    for p in m.parameters():
        p.grad = None
    train_ops.fused_cross_entropy(m(x.to(DEV)), y.to(DEV)).backward()
    m.eval()


@pytest.mark.parametrize("which", ["sgd", "adam_foreach", "fused_adam"])
def test_optimizer_step_between_eval_calls(base, which):
    """Gradients from the training path, one optimizer step, eval logits against the oracle on ``model.state_dict()``.  The
    eval call BEFORE the step already runs on the running statistics the training forward updated, so the step alone is the
    mutation the second eval call must see.  Step sizes: on the oracle alone, SGD at lr 0.01 and a first Adam step at lr 2e-4
    (every weight moves by lr) each move the logits by more than 0.1 while keeping them below 1."""
    m = _model(base["sd"])
    m.gru.dropout = 0.0
    x, y = base["x"], synth.synth_labels(3, mr.NUM_CLASSES, seed=3)
    _assert_close(m(x.to(DEV)), base["ref"], "before training")
    _train_backward(m, x, y)
    opt = {"sgd": lambda: torch.optim.SGD(m.parameters(), lr=0.01),
           "adam_foreach": lambda: torch.optim.Adam(m.parameters(), lr=2e-4, foreach=True),
           "fused_adam": lambda: FusedAdam(m.parameters(), lr=2e-4)}[which]()
    after_fwd = _check_now(m, x, base["ref"], "after the training forward (running statistics)")
    opt.step()
    _check_now(m, x, after_fwd, f"after {which}.step()")


def test_ema_swap_in_and_out(base):
    m = _model(base["sd"])
    m.gru.dropout = 0.0
    x, y = base["x"], synth.synth_labels(3, mr.NUM_CLASSES, seed=3)
    opt = FusedAdam(m.parameters(), lr=4e-4, ema_decay=0.5)
    _train_backward(m, x, y)
    opt.step()
    live = _check_now(m, x, base["ref"], "live weights after the step")
    with opt.swapped_ema():
        shadow = _check_now(m, x, live, "EMA weights swapped in")
    _check_now(m, x, shadow, "live weights swapped back")
    _assert_close(m(x.to(DEV)), live, "live weights, as before the swap")


# ---- e. the training consumer -----------------------------------------------------------------------------------------------
def test_training_step_after_head_swap():
    """One training step at 31 classes, a new 6-class head, another step: logits, loss and every gradient against the oracle
    at the tolerances of test_train_gpu.py::test_ragged_training_step_vs_oracle (no stage views at this shape: loss 1e-5, logits
    2e-5, gradients 2e-3 of the tensor's RMS, 2e-2 on the conv / BatchNorm tensors whose pooling ties the plain oracle cannot
    pin).  The gradient buffer of the first step must not be written by the second."""
    import cases
    bsz, t = 5, 96
    x = cases.varied_features(bsz, t, seed=77 + bsz)
    m = CNNAudioGRU(mr.NUM_CLASSES)
    m.load_state_dict(mr.base_state_dict())
    m = m.to(DEV).train()
    m.gru.dropout = 0.0
    train_ops.fused_cross_entropy(m(x.to(DEV)), synth.synth_labels(bsz, mr.NUM_CLASSES, seed=bsz).to(DEV)).backward()
    torch.cuda.synchronize()
    old = {n: p.grad for n, p in m.named_parameters()}
    old_values = {n: g.clone() for n, g in old.items()}
    assert old["fc.weight"].shape == (mr.NUM_CLASSES, 512)

    mr.swap_head(m, DEV)
    for p in m.parameters():
        p.grad = None
    sd_now = mr.cpu_state(m)
    y = synth.synth_labels(bsz, mr.NEW_CLASSES, seed=bsz)
    logits = m(x.to(DEV))
    loss = train_ops.fused_cross_entropy(logits, y.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    ref_loss, ref_grads, _, ref_logits = model_ref.loss_and_grads(sd_now, x, y)
    assert logits.shape == (bsz, mr.NEW_CLASSES)
    assert abs(loss.item() - ref_loss.item()) < 1e-5
    assert (logits.detach().cpu() - ref_logits).abs().max() < 2e-5
    assert m.fc.weight.grad.shape == (mr.NEW_CLASSES, 512) and m.fc.bias.grad.shape == (mr.NEW_CLASSES,)
    for name, p in m.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape, name
        if ref_grads[name].abs().max() <= 1e-7:
            continue
        e = _rel(p.grad, ref_grads[name])[0]
        print(f"{name}: gradient error {e:.2e}")
        assert e < (2e-2 if name.startswith(("conv", "bn")) else 2e-3), (name, e)
    for n, g in old.items():
        assert torch.equal(g, old_values[n]), f"{n}: the first step's gradient was overwritten through a stale view"


# ---- f. more workspaces than prepare entries --------------------------------------------------------------------------------
def test_five_workspaces_over_four_prepare_entries(base):
    """The handle remembers four prepared workspaces; four pipeline slots and a second model make five, so every round evicts
    an entry.  Two rounds, an in-place update of the first model's ``conv2.weight``, two more rounds."""
    from sir_amd.pipeline import BatchPipeline
    m = _model(base["sd"])
    sd_b = synth.synth_state_dict(mr.NUM_CLASSES, seed=1)
    other = _model(sd_b)
    pipe = BatchPipeline(m, n_streams=4)
    xs = [mr.features(seed=21 + i) for i in range(4)]
    xb = mr.features(seed=30)
    ref_other = _oracle(sd_b, xb)

    def rounds(sd, tag):
        refs = [_oracle(sd, x) for x in xs]
        for r in range(2):
            outs = [pipe.infer(i, x.to(DEV), want_argmax=False) for i, x in enumerate(xs)]
            pipe.synchronize()
            got_other = other(xb.to(DEV))
            for i, (got, ref) in enumerate(zip(outs, refs)):
                _assert_close(got, ref, f"{tag}, round {r}, slot {i}")
            _assert_close(got_other, ref_other, f"{tag}, round {r}, second model")
        return refs

    before = rounds(base["sd"], "before")
    with torch.no_grad():
        mr.mutate_(m.conv2.weight, "conv2.weight", base["sd"]["conv2.weight"])
    sd2 = mr.cpu_state(m)
    for ref_new, ref_old in zip([_oracle(sd2, x) for x in xs], before):
        _assert_moved(ref_new, ref_old, "conv2.weight")
    rounds(sd2, "after")
    assert len({id(w) for w in pipe.workspaces} | {id(other._ws)}) == 5


# ---- g. the C contract ------------------------------------------------------------------------------------------------------
def test_version_zero_always_prepares(base):
    """``sir_model_set_weights_version(h, 0)`` means "prepare on every call": a prepared tensor rewritten through ``.data``
    between two direct ``sir_model_infer`` calls on one workspace is seen by the second."""
    m = _model(base["sd"])
    x = base["x"].to(DEV)
    lib, h = _native.lib(), get_featurizer().handle
    bsz, _, t = x.shape
    ws = torch.empty(lib.sir_model_workspace_bytes(h, bsz, t, 0), dtype=torch.uint8, device=DEV)
    w, keep = ops.weights_struct(m)

    def infer():
        logits = torch.empty(bsz, w.num_classes, device=DEV)
        _native.check(lib.sir_model_set_weights_version(h, 0), "sir_model_set_weights_version")
        rc = lib.sir_model_infer(h, C.byref(w), x.data_ptr(), bsz, t, logits.data_ptr(), None, ws.data_ptr(), ws.numel(),
                                 _native.current_stream_ptr())
        _native.check(rc, "sir_model_infer")
        return logits

    _assert_close(infer(), base["ref"], "first call")
    key = "gru.weight_hh_l0"
    mr.mutate_(mr.tensor_of(m, key).data, key, base["sd"][key])
    sd2, ref, _ = _mutated_ref(base, key)
    assert torch.equal(mr.tensor_of(m, key).detach().cpu(), sd2[key])
    _assert_moved(ref, base["ref"], key)
    _assert_close(infer(), ref, "second call")
    del keep
