"""Host twin of tests/test_weight_mutation_gpu.py: the two caches ``ops.cached_weights`` / ``ops.weights_version`` keep on a model
must follow every route that replaces its tensors, on a CPU model (``ops._f32c`` patched to accept CPU tensors; it still
refuses anything but contiguous float32).  Nothing is launched here: the GPU file checks the logits."""
import copy

import pytest
import torch

import mutation_ref as mr
from sir_amd import _native, ops
from sir_amd.models.models import CNNAudioGRU


class _Ws:
    generation = 1


@pytest.fixture(autouse=True)
def _cpu_tensors_pass(monkeypatch):
    def f32c(t, name):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise _native.SirError(f"{name} must be contiguous float32")
        return t
    monkeypatch.setattr(ops, "_f32c", f32c)


def _model():
    m = CNNAudioGRU(mr.NUM_CLASSES)
    m.load_state_dict(mr.base_state_dict())
    return m.eval()


def _struct_pointers(w):
    """reference key name -> the address ``sir_model_weights`` holds for it"""
    out = {"attention.weight": w.attn_w, "attention.bias": w.attn_b, "fc.weight": w.fc_w, "fc.bias": w.fc_b}
    for i in range(3):
        out.update({f"conv{i + 1}.weight": w.conv_w[i], f"bn{i + 1}.weight": w.bn_w[i], f"bn{i + 1}.bias": w.bn_b[i],
                    f"bn{i + 1}.running_mean": w.bn_mean[i], f"bn{i + 1}.running_var": w.bn_var[i]})
    for i, suf in enumerate(ops.GRU_SUFFIXES):
        out.update({"gru.weight_ih" + suf: w.gru_w_ih[i], "gru.weight_hh" + suf: w.gru_w_hh[i],
                    "gru.bias_ih" + suf: w.gru_b_ih[i], "gru.bias_hh" + suf: w.gru_b_hh[i]})
    return out


def _current_pointers(m):
    return {k: v.data_ptr() for k, v in m.state_dict(keep_vars=True).items() if v.is_floating_point()}


def _snapshot(m):
    """what the next call would hand the library: (pointers by name, num_classes, fingerprint, token)"""
    w, keep = ops.cached_weights(m)
    return _struct_pointers(w), w.num_classes, ops.weights_version(m, keep, _Ws()), m._sir_token


@pytest.mark.parametrize("route", list(mr.ROUTES))
def test_caches_follow_replaced_tensors(route):
    m = _model()
    ptrs, ncls, version, token = _snapshot(m)
    assert ptrs == _current_pointers(m) and ncls == mr.NUM_CLASSES
    mr.ROUTES[route](m, "cpu")
    ptrs2, ncls2, version2, token2 = _snapshot(m)
    assert ptrs2 == _current_pointers(m), [k for k in ptrs2 if ptrs2[k] != _current_pointers(m)[k]]
    assert ptrs2 != ptrs                                   # the route did replace a tensor
    assert ncls2 == m.fc.weight.shape[0] == (mr.NEW_CLASSES if route == "head_swap" else mr.NUM_CLASSES)
    assert version2 != version and token2 != token


def test_half_is_refused_by_name_and_float_recovers():
    m = _model()
    _, _, version, _ = _snapshot(m)
    m.half()
    with pytest.raises(_native.SirError, match=r"conv1\.weight must be contiguous float32"):
        ops.cached_weights(m)
    m.float()
    ptrs, _, version2, _ = _snapshot(m)
    assert ptrs == _current_pointers(m) and version2 != version


def test_removed_tensor_is_refused_by_name():
    m = _model()
    _snapshot(m)
    m.attention.bias = None
    with pytest.raises(_native.SirError, match=r"attention\.bias"):
        ops.cached_weights(m)


@pytest.mark.parametrize("when", ["before_first_call", "after_one_call"])
def test_deepcopy_shares_nothing(when):
    m = _model()
    if when == "after_one_call":
        _snapshot(m)                                       # a populated cache: ctypes pointers cannot be copied
        m._sir_train = {"grads": object(), "ws": ops.Workspace(), "token": m._sir_token}
    c = copy.deepcopy(m)
    assert "_sir_train" not in c.__dict__ and c._sir_wcache is None
    assert c._ws is not m._ws and isinstance(c._ws, ops.Workspace)
    (pm, _, vm, tm), (pc, _, vc, tc) = _snapshot(m), _snapshot(c)
    assert tm != tc and vm != vc
    assert pm == _current_pointers(m) and pc == _current_pointers(c) and not set(pm.values()) & set(pc.values())
    assert ops.cached_weights(m)[0] is not ops.cached_weights(c)[0]
    for (k, a), (_, b) in zip(m.state_dict().items(), c.state_dict().items()):
        assert torch.equal(a, b), k
    # each object follows its own changes only
    with torch.no_grad():
        c.conv3.weight.add_(1.0)
    assert _snapshot(m)[2] == vm and _snapshot(c)[2] != vc
    mr.swap_head(m, "cpu")
    pm2, ncls, vm2, tm2 = _snapshot(m)
    assert ncls == mr.NEW_CLASSES and pm2 == _current_pointers(m) and vm2 != vm and tm2 != tm
    assert _snapshot(c)[0] == pc and _snapshot(c)[1] == mr.NUM_CLASSES


def test_pickle_round_trip_drops_the_caches():
    import pickle
    m = _model()
    _snapshot(m)
    c = pickle.loads(pickle.dumps(m))
    assert c._sir_wcache is None and c._sir_token != m._sir_token and c._ws is not m._ws
    assert _snapshot(c)[0] == _current_pointers(c)


def test_unchanged_model_stays_on_the_fast_path(monkeypatch):
    """1000 calls on a model nobody touched: one ``weights_struct``, the same struct object, pointers, fingerprint and token."""
    calls = []
    real = ops.weights_struct
    monkeypatch.setattr(ops, "weights_struct", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    m = _model()
    first = ops.cached_weights(m)
    snap = _snapshot(m)
    for _ in range(1000):
        cache = ops.cached_weights(m)
        assert cache is first
        assert ops.weights_version(m, cache[1], _Ws()) == snap[2]
    assert _snapshot(m) == snap and len(calls) == 1
    # in-place updates keep the struct (the addresses hold) and move the fingerprint alone
    with torch.no_grad():
        m.fc.bias.add_(1.0)
    assert ops.cached_weights(m) is first and len(calls) == 1
    assert _snapshot(m)[2] != snap[2] and _snapshot(m)[3] == snap[3]
    v = _snapshot(m)[2]
    m.fc.bias.data.add_(1.0)                                # no version counter moves ...
    assert _snapshot(m)[2] == v
    m.weights_changed()                                     # ... the documented call does
    assert _snapshot(m)[2] != v and ops.cached_weights(m) is first and len(calls) == 1


def test_training_state_follows_the_token():
    """``train_ops._train_state``: the gradient buffer is rebuilt (never reused) once the parameter set changed."""
    from sir_amd import train_ops
    m = _model()
    ops.cached_weights(m)
    st = train_ops._train_state(m)
    assert train_ops._train_state(m) is st
    old_flat = st["grads"].flat
    mr.swap_head(m, "cpu")
    ops.cached_weights(m)
    st2 = train_ops._train_state(m)
    assert st2 is not st and st2["grads"].flat is not old_flat and st2["ws"] is st["ws"]
    views = dict(zip(st2["grads"].names, st2["grads"].views))
    assert views["fc.weight"].shape == (mr.NEW_CLASSES, 512) and views["fc.bias"].shape == (mr.NEW_CLASSES,)
    assert st2["grads"].flat.numel() == sum(p.numel() for p in m.parameters())


def test_removed_sub_module_is_refused_by_name():
    m = _model()
    _snapshot(m)
    del m.fc
    with pytest.raises(_native.SirError, match="fc"):
        ops.cached_weights(m)
