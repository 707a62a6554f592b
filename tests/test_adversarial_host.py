"""Host (no GPU): the numpy restatement of ``sir_adv_step`` checks itself, and everything of adversarial training that is
decided before a device call -- argument validation, the default step sizes, the ``adversarial`` YAML key, the host draws
of ``train_ops.Adversary`` and their place in the run state."""
import random

import numpy as np
import pytest
import torch
import torch.nn as nn

import adv_ref
from sir_amd import _native, explain, run_state, train_ops
from sir_amd.scripts import train as tr

F32 = np.float32


# ---- adv_ref ----------------------------------------------------------------------------------------------------------
def test_uniform_matches_the_dropout_mask_threshold():
    for seed in (0, 1, 0x9E3779B97F4A7C15, (1 << 64) - 1):
        u = adv_ref.check_uniform_against_dropout_keep(seed, 4096)
        assert np.array_equal(u * F32(16777216.0), np.floor(u * F32(16777216.0)))        # multiples of 2^-24
    assert 0.45 < adv_ref.uniform24(7, 1 << 16).mean() < 0.55


def test_ref_zero_ordering_and_nan_rules():
    pz, nz, nan = F32(0.0), F32(-0.0), F32(np.nan)
    a = np.array([pz, nz, nz, nan, F32(1.0)], dtype=F32)
    b = np.array([nz, pz, nz, F32(2.0), nan], dtype=F32)
    assert adv_ref.fmaxf(a, b).view(np.uint32).tolist() == [0, 0, 0x80000000, 0x40000000, 0x3F800000]
    assert adv_ref.fminf(a, b).view(np.uint32).tolist() == [0x80000000, 0x80000000, 0x80000000, 0x40000000, 0x3F800000]
    assert adv_ref.sign_step(np.array([1.0, -1.0, 0.0, -0.0, np.nan], dtype=F32), 0.5).tolist() == [0.5, -0.5, 0.0, 0.0, 0.0]


def test_ref_step_projects_keeps_and_copies_bits():
    rng = np.random.default_rng(0)
    x0 = rng.standard_normal((3, 64, 10)).astype(F32)
    x0[:, :, 7:] = 0.0                                   # padding
    x0[0, :, 2] = -0.0                                   # data
    x0[1, 5, 3] = np.nan
    x0[1, 6, 3] = -0.0
    g = rng.standard_normal(x0.shape).astype(F32)
    g[0, 0, 0] = 0.0
    g[0, 1, 0] = np.nan
    active = np.array([1, 0, 1], dtype=np.int32)
    out = adv_ref.adv_step(x0, x0, g, eps=0.1, alpha=0.25, active=active)
    bits0, bits = x0.view(np.uint32), out.view(np.uint32)
    assert np.array_equal(bits[1], bits0[1])                                             # inactive: NaN payload and -0.0 kept
    assert np.array_equal(bits[:, :, 7:], bits0[:, :, 7:])                               # zero columns kept
    assert out[0, 0, 0] == x0[0, 0, 0] and out[0, 1, 0] == x0[0, 1, 0]                   # zero / NaN gradient: no move
    live = np.ones(x0.shape, dtype=bool)
    live[1] = False
    live[:, :, 7:] = False
    live[0, :2, 0] = False
    assert np.array_equal(out[live], np.where(g > 0, x0 + F32(0.1), x0 - F32(0.1))[live])   # alpha > eps: lands on the ball
    assert (np.abs(out[0, :, 2]) == F32(0.1)).all()                                      # the -0.0 column is perturbed
    loose = adv_ref.adv_step(x0, x0, g, eps=0.1, alpha=0.25, active=active, keep_zero_columns=False)
    assert (np.abs(loose[0, :, 7:]) == F32(0.1)).all() and np.array_equal(loose.view(np.uint32)[1], bits0[1])
    start = adv_ref.adv_step(x0, eps=0.1, active=active, seed=3)
    moved = np.isfinite(x0) & (np.arange(10) < 7)[None, None, :] & (active != 0)[:, None, None]
    assert (np.abs(start[moved].astype(np.float64) - x0[moved]) <= 0.1 * (1 + 2.0 ** -20) + np.abs(x0[moved]) * 2.0 ** -23).all()
    assert (start[moved] != x0[moved]).mean() > 0.99
    assert np.array_equal(start.view(np.uint32)[1], bits0[1]) and np.array_equal(start[:, :, 7:], x0[:, :, 7:])
    u = adv_ref.uniform24(3, x0.size).reshape(x0.shape)
    assert start[2, 4, 1] == min(max(x0[2, 4, 1] + F32(0.1) * (F32(2) * u[2, 4, 1] - F32(1)), x0[2, 4, 1] - F32(0.1)), x0[2, 4, 1] + F32(0.1))
    same = adv_ref.adv_step(x0, x0, g, eps=0.0, alpha=0.0, active=None, keep_zero_columns=False)
    ordinary = ~np.isnan(x0) & (bits0 != 0x80000000)
    assert np.array_equal(same.view(np.uint32)[ordinary], bits0[ordinary])               # eps 0: the bits of x0 (no -0.0, no NaN)


# ---- validation before any device call --------------------------------------------------------------------------------
def _bar_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(_native, "lib", no_device)
    monkeypatch.setattr(_native, "require_hip", no_device)
    monkeypatch.setattr(_native, "current_stream_ptr", no_device)


def test_adv_step_validates_before_any_device_call(monkeypatch):
    _bar_device(monkeypatch)
    x = torch.zeros(2, 64, 9)
    bad = [
        (dict(x0=x, x=x, g=x, eps=-1.0, alpha=0.1), ValueError, "eps"),
        (dict(x0=x, x=x, g=x, eps=float("nan"), alpha=0.1), ValueError, "eps"),
        (dict(x0=x, x=x, g=x, eps=0.1, alpha=-0.1), ValueError, "alpha"),
        (dict(x0=x, x=x, g=x, eps=0.1, alpha=float("nan")), ValueError, "alpha"),
        (dict(x0=x, x=x, g=None, eps=0.1, alpha=0.1), ValueError, "without g"),
        (dict(x0=x, x=None, g=x, eps=0.1, alpha=0.1), ValueError, "needs the iterate"),
        (dict(x0=x.double(), x=None, g=None, eps=0.1, alpha=0.1), ValueError, "float32"),
        (dict(x0=torch.zeros(2, 63, 9), x=None, g=None, eps=0.1, alpha=0.1), ValueError, "expected"),
        (dict(x0=torch.zeros(2, 2, 64, 9), x=None, g=None, eps=0.1, alpha=0.1), ValueError, "expected"),
        (dict(x0=x, x=x, g=torch.zeros(2, 64, 8), eps=0.1, alpha=0.1), ValueError, "does not match"),
        (dict(x0=x, x=x, g=x, eps=0.1, alpha=0.1), _native.SirError, "HIP device"),       # host tensors: no CPU path
    ]
    for kw, exc, match in bad:
        with pytest.raises(exc, match=match):
            train_ops.adv_step(**kw)


def test_adversary_and_pgd_validate_before_any_device_call(monkeypatch):
    _bar_device(monkeypatch)
    for kw in (dict(eps=-0.1), dict(eps=float("nan")), dict(eps=0.1, steps=0), dict(eps=0.1, prob=1.5), dict(eps=0.1, prob=-0.1),
               dict(eps=0.1, alpha=-1.0)):
        with pytest.raises(ValueError):
            train_ops.Adversary(**kw)
    model = nn.Linear(2, 2)
    with pytest.raises(_native.SirError, match="HIP device"):
        train_ops.Adversary(0.1)(model, torch.zeros(2, 64, 9), lambda out: out.sum())
    with pytest.raises(ValueError, match="float32"):
        train_ops.Adversary(0.1)(model, torch.zeros(2, 64, 9).double(), lambda out: out.sum())
    x, y = torch.zeros(2, 64, 9), torch.zeros(2, dtype=torch.int64)
    for kw, exc in ((dict(eps=-1.0), ValueError), (dict(eps=0.1, steps=0), ValueError), (dict(eps=0.1, alpha=-1.0), ValueError),
                    (dict(eps=0.1, seed=-1), ValueError), (dict(eps=0.1, lengths=[9, 9]), ValueError), (dict(eps=0.1), _native.SirError)):
        with pytest.raises(exc):
            explain.pgd(model, x, y, **kw)
    with pytest.raises(ValueError, match="T >= 8"):
        explain.pgd(model, torch.zeros(2, 64, 7), y, 0.1)


# ---- default alpha ----------------------------------------------------------------------------------------------------
def test_default_alpha_rules():
    eps = 0.08
    assert train_ops.Adversary(eps, steps=1, random_start=False).alpha == eps
    assert train_ops.Adversary(eps, steps=1, random_start=True).alpha == 1.25 * eps
    assert train_ops.Adversary(eps, steps=4, random_start=True).alpha == 2.5 * eps / 4
    assert train_ops.Adversary(eps, steps=4, random_start=False).alpha == 2.5 * eps / 4
    assert train_ops.Adversary(eps, alpha=0.01, steps=4).alpha == 0.01
    assert train_ops.Adversary(0.0, steps=2).alpha == 0.0
    for steps in (1, 2, 7):
        for rs in (False, True):
            assert train_ops.default_adv_alpha(eps, steps, rs) == adv_ref.default_alpha(eps, steps, rs)
    a = train_ops.Adversary(eps)                          # the defaults of the YAML key
    assert (a.steps, a.random_start, a.prob) == (1, True, 1.0)


# ---- YAML -------------------------------------------------------------------------------------------------------------
def test_adversarial_yaml_key():
    assert tr.adversarial_options({}) is None and tr.adversarial_options({"adversarial": None}) is None
    got = tr.adversarial_options({"adversarial": {"eps": 0.05}})
    assert got == {"eps": 0.05, "alpha": None, "steps": 1, "random_start": True, "prob": 1.0, "validate": False}
    got = tr.adversarial_options({"adversarial": {"eps": "1e-2", "alpha": 0.004, "steps": 3, "random_start": False, "prob": 0.5,
                                                  "validate": True}})
    assert got == {"eps": 0.01, "alpha": 0.004, "steps": 3, "random_start": False, "prob": 0.5, "validate": True}
    assert tr.adversarial_options({"adversarial": {"eps": 0}})["eps"] == 0.0
    for spec, match in (({"eps": -0.1}, "eps"), ({"eps": 0.1, "steps": 0}, "steps"), ({"eps": 0.1, "prob": 1.01}, "prob"),
                        ({"eps": 0.1, "prob": -0.5}, "prob"), ({"eps": 0.1, "radius": 2}, "unknown keys"), ({"steps": 2}, "eps"),
                        ({"eps": 0.1, "alpha": -1}, "alpha"), ([0.1], "mapping")):
        with pytest.raises(ValueError, match=match):
            tr.adversarial_options({"adversarial": spec})
    assert "adversarial" in run_state.STATE_KEYS


# ---- determinism of the draws ---------------------------------------------------------------------------------------
def test_adversary_draws_are_a_function_of_the_seed():
    a, b, ref = train_ops.Adversary(0.1, prob=0.5, seed=11), train_ops.Adversary(0.1, prob=0.5, seed=11), adv_ref.AdversaryDraws(0.5, 11)
    seq = [a.draw(n) for n in (8, 3, 8)]
    for (fa, sa), n in zip(seq, (8, 3, 8)):
        fb, sb = b.draw(n)
        fr, sr = ref.draw(n)
        assert fa.dtype == torch.int32 and torch.equal(fa, fb) and fa.tolist() == fr and sa == sb == sr and 0 <= sa < 1 << 64
    assert 0 < sum(int(f.sum()) for f, _ in seq) < 19                                    # prob 0.5: some of each
    other = train_ops.Adversary(0.1, prob=0.5, seed=12)
    assert [other.draw(n)[1] for n in (8, 3, 8)] != [s for _, s in seq]
    state = a.rng.getstate()
    want = [a.draw(5) for _ in range(3)]
    c = train_ops.Adversary(0.1, prob=0.5, seed=99)
    c.rng.setstate(state)
    for (fw, sw), (fc, sc) in zip(want, [c.draw(5) for _ in range(3)]):
        assert torch.equal(fw, fc) and sw == sc
    assert train_ops.Adversary(0.1, prob=1.0).draw(6)[0].tolist() == [1] * 6
    assert train_ops.Adversary(0.1, prob=0.0).draw(6)[0].tolist() == [0] * 6
    assert isinstance(a.rng, random.Random)


# ---- run state --------------------------------------------------------------------------------------------------------
def _stand_in(seed=0):
    torch.manual_seed(seed)
    model = nn.Sequential(nn.Linear(4, 3), nn.BatchNorm1d(3))
    return model, torch.optim.Adam(model.parameters(), lr=0.01)


def test_run_state_carries_the_adversary_rng(tmp_path):
    before = train_ops.dropout_step()
    try:
        model, opt = _stand_in()
        adv = train_ops.Adversary(0.05, steps=2, prob=0.5, seed=4)
        adv.draw(8)
        path = tmp_path / run_state.LATEST
        run_state.save_run_state(path, model, opt, adversary=adv, epoch=0, config={"adversarial": {"eps": 0.05}, "epochs": 3})
        raw = torch.load(path, weights_only=False)
        assert raw["per_rank"][0]["adversary_rng"] == adv.rng.getstate() and raw["per_rank"][0]["mixup_rng"] is None
        assert raw["config"] == {"adversarial": {"eps": 0.05}}
        want = [adv.draw(8) for _ in range(3)]
        model2, opt2 = _stand_in(seed=1)
        adv2 = train_ops.Adversary(0.05, steps=2, prob=0.5, seed=77)
        got = run_state.load_run_state(path, model2, opt2, adversary=adv2, config={"adversarial": {"eps": 0.1}})
        assert got["config_changed"] == ["adversarial"]
        for (fw, sw), (fg, sg) in zip(want, [adv2.draw(8) for _ in range(3)]):
            assert torch.equal(fw, fg) and sw == sg
        # presence must agree, both ways
        with pytest.raises(ValueError, match="had a adversary.*has none"):
            run_state.load_run_state(path, model2, opt2)
        plain = tmp_path / "plain.pt"
        run_state.save_run_state(plain, model, opt, epoch=0)
        assert torch.load(plain, weights_only=False)["per_rank"][0]["adversary_rng"] is None
        with pytest.raises(ValueError, match="had no adversary.*has one"):
            run_state.load_run_state(plain, model2, opt2, adversary=adv2)
        # a file written before the key existed reads as "no adversary"
        old = torch.load(plain, weights_only=False)
        del old["per_rank"][0]["adversary_rng"]
        torch.save(old, tmp_path / "old.pt")
        assert run_state.load_run_state(tmp_path / "old.pt", model2, opt2)["epoch"] == 0
        with pytest.raises(ValueError, match="adversary"):
            run_state.load_run_state(tmp_path / "old.pt", model2, opt2, adversary=adv2)
    finally:
        train_ops.set_dropout_step(before)


# ---- the adversary rides on the model -------------------------------------------------------------------------------
def test_adversary_rides_on_the_model_and_the_epoch_signatures_stay():
    import inspect
    model = nn.Linear(2, 2)
    assert train_ops.adversary_of(model) is None
    adv = train_ops.Adversary(0.1)
    assert train_ops.set_adversary(model, adv) is adv and train_ops.adversary_of(model) is adv
    assert "_sir_adversary" not in model.state_dict()
    train_ops.set_adversary(model, None)
    assert train_ops.adversary_of(model) is None
    with pytest.raises(TypeError):
        train_ops.set_adversary(model, object())
    assert "adversary" not in inspect.signature(tr.train_epoch).parameters
    assert "adversary" not in inspect.signature(tr.train_epoch_waveforms).parameters
    assert "adversary" in inspect.signature(run_state.save_run_state).parameters
    assert list(inspect.signature(run_state.load_run_state).parameters)[-1] == "adversary"
