"""CPU: the run-management layer without a GPU -- the ``lr_schedule`` builder against torch's scheduler classes built by
hand, ``run_state`` save / load on a CPU stand-in (atomic write, world-size and layout mismatches, mixup and dropout
counter continuation), and the option parsing of ``train()`` (nothing new is on by default)."""
import os

import pytest
import torch
import torch.nn as nn
from torch.optim import lr_scheduler as sched

from sir_amd import run_state, train_ops
from sir_amd.scripts import train as tr

BASE_LR, WARM, TOTAL = 0.05, 3, 12


def _sgd():
    return torch.optim.SGD([nn.Parameter(torch.zeros(3))], lr=BASE_LR)


def _by_hand(opt, kind):
    warm = sched.LinearLR(opt, start_factor=1.0 / (WARM + 1), end_factor=1.0, total_iters=WARM)
    if kind == "cosine":
        main = sched.CosineAnnealingLR(opt, T_max=TOTAL - WARM, eta_min=1e-4)
    elif kind == "step":
        main = sched.StepLR(opt, step_size=4, gamma=0.5)
    else:
        main = sched.LambdaLR(opt, lambda step: 1.0)
    return sched.SequentialLR(opt, [warm, main], milestones=[WARM])


SPECS = {"constant": {"kind": "constant", "warmup_steps": WARM},
         "cosine": {"kind": "cosine", "warmup_steps": WARM, "total_steps": TOTAL, "min_lr": 1e-4},
         "step": {"kind": "step", "warmup_steps": WARM, "step_size": 4, "gamma": 0.5}}


def _run(opt, s, n):
    lrs = []
    for _ in range(n):
        lrs.append(opt.param_groups[0]["lr"])
        opt.step()
        s.step()
    return lrs


@pytest.mark.parametrize("kind", ["constant", "cosine", "step"])
def test_lr_schedule_builder_equals_torch_classes_and_round_trips(kind):
    opt_a, opt_b = _sgd(), _sgd()
    got = _run(opt_a, tr.build_lr_scheduler(opt_a, dict(SPECS[kind])), TOTAL)
    want = _run(opt_b, _by_hand(opt_b, kind), TOTAL)
    assert got == want                                           # Python floats, ==
    assert got[0] == BASE_LR / (WARM + 1) and got[WARM] == BASE_LR and len(set(got[:WARM + 1])) == WARM + 1
    if kind == "cosine":
        assert got[-1] < got[WARM] and min(got[WARM:]) >= 1e-4
    if kind == "constant":
        assert set(got[WARM:]) == {BASE_LR}
    # state_dict -> fresh optimizer + scheduler -> the same continuation
    opt_c = _sgd()
    s_c = tr.build_lr_scheduler(opt_c, dict(SPECS[kind]))
    head = _run(opt_c, s_c, 5)
    saved = {"opt": opt_c.state_dict(), "sched": s_c.state_dict()}
    opt_d = _sgd()
    s_d = tr.build_lr_scheduler(opt_d, dict(SPECS[kind]))
    opt_d.load_state_dict(saved["opt"])
    s_d.load_state_dict(saved["sched"])
    assert head + _run(opt_d, s_d, TOTAL - 5) == want


def test_scheduler_rides_on_the_optimizer_step():
    """``step_scheduler_with``: every ``optimizer.step()`` steps the scheduler once, whoever calls it."""
    opt_a, opt_b = _sgd(), _sgd()
    s_a = tr.build_lr_scheduler(opt_a, dict(SPECS["cosine"]))
    handle = tr.step_scheduler_with(opt_a, s_a)
    got = []
    for _ in range(TOTAL):
        got.append(opt_a.param_groups[0]["lr"])
        opt_a.step()
    assert got == _run(opt_b, _by_hand(opt_b, "cosine"), TOTAL)
    handle.remove()
    before = opt_a.param_groups[0]["lr"]
    opt_a.step()
    assert opt_a.param_groups[0]["lr"] == before


def test_lr_schedule_without_warmup_and_bad_specs():
    opt = _sgd()
    s = tr.build_lr_scheduler(opt, {"kind": "step", "step_size": 2, "gamma": 0.1})
    assert isinstance(s, sched.StepLR)
    assert tr.build_lr_scheduler(_sgd(), None) is None and tr.build_lr_scheduler(_sgd(), {}) is None
    for bad in ({"kind": "linear"}, {"kind": "cosine"}, {"kind": "step"}, {"kind": "constant", "warmup": 3},
                {"kind": "cosine", "warmup_steps": 5, "total_steps": 5}):
        with pytest.raises(ValueError):
            tr.build_lr_scheduler(_sgd(), bad)


def _stand_in(width=4, seed=0):
    torch.manual_seed(seed)
    model = nn.Sequential(nn.Linear(width, 3), nn.BatchNorm1d(3))
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    s = tr.build_lr_scheduler(opt, dict(SPECS["cosine"]))
    return model, opt, s, train_ops.Mixup(0.4, seed=5)


def _advance(model, opt, s, mixup, steps=3):
    for _ in range(steps):
        opt.zero_grad()
        model(torch.randn(8, model[0].in_features)).square().mean().backward()
        opt.step()
        s.step()
        mixup.draw(6)
    opt.zero_grad()


@pytest.fixture
def dropout_counter():
    before = train_ops.dropout_step()
    yield
    train_ops.set_dropout_step(before)


def test_run_state_round_trip_continues_everything(tmp_path, dropout_counter):
    model, opt, s, mixup = _stand_in()
    _advance(model, opt, s, mixup)
    train_ops.set_dropout_step(41)
    path = tmp_path / "ckpt" / run_state.LATEST
    assert run_state.save_run_state(path, model, opt, s, mixup, epoch=2, best_val_acc=0.75, no_improve_count=1,
                                    config={"optimizer": "adamw", "seed": 3, "epochs": 9}) == str(path)
    assert os.listdir(path.parent) == [run_state.LATEST]                       # no temporary file is left behind
    raw = torch.load(path, weights_only=False)
    assert set(raw["model_state_dict"]) == set(model.state_dict())             # the key the checkpoint loaders look under
    assert raw["world_size"] == 1 and raw["config"] == {"optimizer": "adamw", "seed": 3}
    want_draws = [mixup.draw(6) for _ in range(4)]
    want_lr = _run(opt, s, 4)

    train_ops.set_dropout_step(1)                                             # a new process
    model2, opt2, s2, mixup2 = _stand_in(seed=1)
    got = run_state.load_run_state(path, model2, opt2, s2, mixup2, config={"optimizer": "adam", "seed": 3})
    assert (got["epoch"], got["best_val_acc"], got["no_improve_count"]) == (2, 0.75, 1)
    assert got["config_changed"] == ["optimizer"]
    assert train_ops.dropout_step() == 41
    assert next(train_ops._seed_counter) == 41 and train_ops.dropout_step() == 42      # ... and counts on from there
    for (k, a), b in zip(raw["model_state_dict"].items(), model2.state_dict().values()):
        assert torch.equal(a, b), k
    for (pa, la), (pb, lb) in zip(want_draws, [mixup2.draw(6) for _ in range(4)]):
        assert torch.equal(pa, pb) and torch.equal(la, lb)
    assert _run(opt2, s2, 4) == want_lr
    st, st2 = raw["optimizer_state_dict"]["state"], opt2.state_dict()["state"]
    assert len(st) == 4 and all(int(st2[i]["step"]) == int(st[i]["step"]) == 3 and torch.equal(st2[i]["exp_avg"], st[i]["exp_avg"]) for i in st)


def test_dropout_counter_starts_at_one_and_keeps_its_keys(dropout_counter):
    train_ops.set_dropout_step(1)
    assert [next(train_ops._seed_counter) for _ in range(3)] == [1, 2, 3]      # what itertools.count(1) handed out
    assert train_ops.dropout_seed(1, rank=0) == 0x9E3779B97F4A7C15
    with pytest.raises(ValueError):
        train_ops.set_dropout_step(0)


def test_atomic_write_never_leaves_a_partial_target(tmp_path, monkeypatch, dropout_counter):
    model, opt, s, mixup = _stand_in()
    path = tmp_path / run_state.LATEST
    run_state.save_run_state(path, model, opt, s, mixup, epoch=0)
    good = path.read_bytes()
    real_save = torch.save

    def dies_half_way(obj, f, *a, **kw):
        assert os.fspath(f) != str(path)                                      # the target itself is never opened for writing
        real_save(obj, f, *a, **kw)
        with open(f, "r+b") as fh:
            fh.truncate(100)
        raise OSError("disk full")

    monkeypatch.setattr(torch, "save", dies_half_way)
    _advance(model, opt, s, mixup)
    with pytest.raises(OSError):
        run_state.save_run_state(path, model, opt, s, mixup, epoch=1)
    monkeypatch.undo()
    assert path.read_bytes() == good and os.listdir(tmp_path) == [run_state.LATEST]
    model2, opt2, s2, mixup2 = _stand_in(seed=1)
    assert run_state.load_run_state(path, model2, opt2, s2, mixup2)["epoch"] == 0


def test_mismatches_raise_and_name_both_sides(tmp_path, dropout_counter):
    model, opt, s, mixup = _stand_in()
    _advance(model, opt, s, mixup)
    path = tmp_path / run_state.LATEST
    run_state.save_run_state(path, model, opt, s, mixup, epoch=0)
    model2, opt2, s2, mixup2 = _stand_in(seed=1)
    before = {k: v.clone() for k, v in model2.state_dict().items()}
    with pytest.raises(ValueError, match=r"world size 1.*world size 2"):
        run_state.load_run_state(path, model2, opt2, s2, mixup2, rank=0, world=2)
    wide = _stand_in(width=5)
    with pytest.raises(ValueError, match=r"4 tensors / 21 elements.*4 tensors / 24 elements"):
        run_state.load_run_state(path, *wide)
    with pytest.raises(ValueError, match="LR scheduler"):
        run_state.load_run_state(path, model2, opt2, None, mixup2)
    with pytest.raises(ValueError, match="mixup"):
        run_state.load_run_state(path, model2, opt2, s2, None)
    for k, v in model2.state_dict().items():                                  # a refused load changes nothing
        assert torch.equal(v, before[k]), k
    bare = tmp_path / "best_model.pt"
    torch.save(model.state_dict(), bare)
    with pytest.raises(ValueError, match="not a run state"):
        run_state.load_run_state(bare, model2, opt2, s2, mixup2)


def test_default_config_turns_nothing_on():
    cfg = {"batch_size": 8, "lr": 1e-3, "weight_decay": 1e-4, "epochs": 2, "save_path": "ckpt"}
    opts = tr.run_options(cfg)
    assert opts == {"decoupled_weight_decay": False, "ema_decay": None, "ema_warmup": False, "lr_schedule": None,
                    "checkpoint_path": None, "resume_path": None}
    assert tr.build_lr_scheduler(_sgd(), opts["lr_schedule"]) is None
    on = tr.run_options(dict(cfg, optimizer="adamw", ema_decay=0.999, ema_warmup=True, checkpoint_every_epoch=True, resume=True,
                             lr_schedule={"kind": "cosine", "warmup_steps": 10}))
    latest = os.path.join("ckpt", "latest_checkpoint.pt")
    assert on == {"decoupled_weight_decay": True, "ema_decay": 0.999, "ema_warmup": True,
                  "lr_schedule": {"kind": "cosine", "warmup_steps": 10}, "checkpoint_path": latest, "resume_path": latest}
    assert tr.run_options(dict(cfg, resume="elsewhere/run.pt"))["resume_path"] == "elsewhere/run.pt"
    with pytest.raises(ValueError):
        tr.run_options(dict(cfg, optimizer="sgd"))
    with pytest.raises(ValueError):
        tr.run_options(dict(cfg, ema_warmup=True))


def test_fused_adam_rejects_bad_ema_decay_and_keys_state_by_index():
    from sir_amd.optim import FusedAdam
    p = [nn.Parameter(torch.zeros(4))]
    for bad in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            FusedAdam(p, ema_decay=bad)
    opt = FusedAdam(p, ema_decay=0.99, ema_warmup=True, decoupled_weight_decay=True)
    assert opt.ema_decay_at(1) == 2.0 / 11.0 and opt.ema_decay_at(10 ** 6) == 0.99
    assert FusedAdam._key(0) == "_sir_group_0"
    # a state whose flat sizes do not fit raises instead of restarting from zero (host tensors: nothing is launched)
    other = FusedAdam([nn.Parameter(torch.zeros(5))], ema_decay=0.99)
    other._group_state(0)
    with pytest.raises(ValueError, match="4 elements.*5"):
        opt.load_state_dict(other.state_dict())
    plain = FusedAdam([nn.Parameter(torch.zeros(4))])
    plain._group_state(0)
    with pytest.raises(ValueError, match="EMA"):
        opt.load_state_dict(plain.state_dict())
    legacy = plain.state_dict()
    legacy["state"] = {"_sir_group_%d" % id(plain): legacy["state"]["_sir_group_0"]}
    with pytest.raises(ValueError, match="process address"):
        plain.load_state_dict(legacy)
    same = FusedAdam([nn.Parameter(torch.ones(4))], ema_decay=0.99, ema_warmup=True, decoupled_weight_decay=True)
    same._group_state(0)["step"] = 7
    opt.load_state_dict(torch.load(_saved(same.state_dict()), weights_only=False))
    gs = opt._group_state(0)
    assert gs["step"] == 7 and torch.equal(gs["ema"], torch.ones(4)) and gs["offsets"] == [0]


def _saved(obj):
    import io
    buf = io.BytesIO()
    torch.save(obj, buf)
    buf.seek(0)
    return buf
