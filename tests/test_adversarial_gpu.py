"""GPU: ``sir_adv_step`` bit for bit against ``tests/adv_ref.py``, the side-effect-free crafting pass, ``train_ops.Adversary`` inside
``train_epoch``, ``explain.pgd`` / ``robust_accuracy`` and the bit-exact resume of an adversarial run.

Bounds.  Everything the kernel writes is compared with ``==`` on the 32-bit words.  The one comparison against the float64 oracle
(``test_one_step_against_the_float64_oracle``) leaves out the elements whose reference gradient lies below the project's own
gradient bound (``|g_ref| <= GRAD_BOUND * rms(g_ref)``: there the device's sign is not determined), caps their share at 1 % of the
live elements, and asks for bit equality everywhere else.  The ascent test asks for half of the first-order estimate
``eps * |g|_1`` (the float64 oracle gives 0.97 of it on such inputs).
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import adv_ref
import input_grad_ref as ref
from sir_amd import _native, explain, finetune, ops, run_state, synth, train_ops
from sir_amd.featurizer import get_featurizer
from sir_amd.models.models import CNNAudioGRU
from sir_amd.optim import FusedAdam
from sir_amd.scripts import train as tr

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
SENTINEL = 0x7FC0ABCD                     # a NaN payload no arithmetic produces
PAD = 64                                  # sentinel floats in front of and behind every output


@pytest.fixture(scope="module")
def sd():
    return synth.synth_state_dict(31, seed=0)


@pytest.fixture
def new_process():
    before = train_ops.dropout_step()
    train_ops.set_dropout_step(1)
    yield
    train_ops.set_dropout_step(before)


def _model(sd, frozen_bn=(), dropout=0.5):
    m = CNNAudioGRU(31)
    m.load_state_dict(sd)
    m = m.to(DEV).train()
    m.gru.dropout = dropout
    for i in frozen_bn:
        getattr(m, f"bn{i}").eval()
    return m


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy().view(np.uint32)


# ---- 1. the kernel ----------------------------------------------------------------------------------------------------
def _kernel_inputs(bsz, t, seed):
    """x0 with a trailing run of zero columns, a zero column in the middle, a column of -0.0, a column with one non-zero value,
    a zero row (a frequency band); a gradient with exact zeros and NaNs; with B >= 2 an inactive row holding -0.0 and a NaN."""
    rng = np.random.default_rng(seed)
    x0 = rng.standard_normal((bsz, 64, t)).astype(F32)
    x0[:, :, t - 3:] = 0.0
    x0[:, :, 2] = 0.0
    x0[:, :, 1] = -0.0
    x0[:, :, 3] = 0.0
    x0[:, 10, 3] = 0.75
    x0[:, 7, :] = 0.0                                    # (also in column 1: one +0.0 among -0.0 is still data)
    x = (x0 + rng.uniform(-0.04, 0.04, x0.shape).astype(F32)).astype(F32)
    x[:, :, 1] = x0[:, :, 1]
    g = rng.standard_normal(x0.shape).astype(F32)
    g[rng.random(x0.shape) < 0.05] = 0.0
    g[rng.random(x0.shape) < 0.02] = np.nan
    g[0, 0, 0], g[0, 1, 0], g[0, 2, 0] = 0.0, -0.0, np.nan
    active = None
    if bsz >= 2:
        active = (rng.random(bsz) < 0.7).astype(np.int32)
        active[0], active[1] = 1, 0
        x0[1, 4, 4], x0[1, 5, 4] = -0.0, np.nan
        x0[1, 6, 4:6] = np.array([0x7FC12345, 0xFF800001], dtype=np.uint32).view(F32)      # NaN payloads, one signalling
    return x0, x, g, active


def _framed(n, offset=0):
    """A sentinel-filled buffer and the view of ``n`` floats ``PAD + offset`` floats into it."""
    buf = torch.full((n + 2 * PAD + 4,), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
    return buf, buf[PAD + offset: PAD + offset + n]


def _frame_intact(buf, n, offset=0):
    bits = _bits(buf)
    return (bits[:PAD + offset] == SENTINEL).all() and (bits[PAD + offset + n:] == SENTINEL).all()


@pytest.mark.parametrize("bsz,t", [(1, 8), (3, 37), (3, 50), (4, 24), (257, 24)])
def test_kernel_bits_against_the_host_restatement(bsz, t):
    x0, x, g, active = _kernel_inputs(bsz, t, seed=100 * bsz + t)
    n = x0.size
    dx0, dg = torch.from_numpy(x0).to(DEV), torch.from_numpy(g).to(DEV)
    dact = torch.from_numpy(active).to(DEV) if active is not None else None
    offsets = (0, 1) if (bsz, t) == (4, 24) else (0,)            # 1: t % 4 == 0 with a 4-byte aligned output -> the element form
    for keep in (True, False):
        for eps, alpha in ((0.05, 0.02), (0.05, 0.125), (0.0, 0.0), (0.0, 0.02)):
            for off in offsets:
                tag = (bsz, t, keep, eps, alpha, off)
                # gradient step, out of place
                buf, view = _framed(n, off)
                out = train_ops.adv_step(dx0, torch.from_numpy(x).to(DEV), dg, eps, alpha, active=dact, keep_zero_columns=keep,
                                         out=view.view(bsz, 64, t))
                want = adv_ref.adv_step(x0, x, g, eps, alpha, active=active, keep_zero_columns=keep)
                assert out.data_ptr() == view.data_ptr()
                assert np.array_equal(_bits(out), want.view(np.uint32)), tag
                assert _frame_intact(buf, n, off), tag
                # in place: out is x
                buf, view = _framed(n, off)
                it = view.view(bsz, 64, t)
                it.copy_(torch.from_numpy(x))
                train_ops.adv_step(dx0, it, dg, eps, alpha, active=dact, keep_zero_columns=keep, out=it)
                assert np.array_equal(_bits(it), want.view(np.uint32)), tag
                assert _frame_intact(buf, n, off), tag
                # first step from x0 itself (x is x0)
                first = train_ops.adv_step(dx0, dx0, dg, eps, alpha, active=dact, keep_zero_columns=keep)
                assert np.array_equal(_bits(first), adv_ref.adv_step(x0, x0, g, eps, alpha, active=active,
                                                                     keep_zero_columns=keep).view(np.uint32)), tag
                # random start
                buf, view = _framed(n, off)
                seed = (0x9E3779B97F4A7C15 * (t + 1) + bsz) % (1 << 64)
                start = train_ops.adv_step(dx0, None, None, eps, alpha, active=dact, seed=seed, keep_zero_columns=keep,
                                           out=view.view(bsz, 64, t))
                assert np.array_equal(_bits(start), adv_ref.adv_step(x0, eps=eps, active=active, seed=seed,
                                                                     keep_zero_columns=keep).view(np.uint32)), tag
                assert _frame_intact(buf, n, off), tag
    # what the inputs were built to show, on the last (keep False) and a keep True result
    kept = train_ops.adv_step(dx0, dx0, dg, 0.05, 0.125, active=dact, keep_zero_columns=True).cpu().numpy()
    b0 = x0.view(np.uint32)
    assert np.array_equal(kept.view(np.uint32)[:, :, t - 3:], b0[:, :, t - 3:]) and np.array_equal(kept[:, :, 2], x0[:, :, 2])
    moved, signed = np.abs(kept[0]) == F32(0.05), (g[0] > 0) | (g[0] < 0)      # (a zero or NaN gradient moves nothing)
    assert np.array_equal(moved[:, 1], signed[:, 1]) and signed[:, 1].sum() > 32      # the -0.0 column is data
    assert np.array_equal(moved[7, :t - 3], signed[7, :t - 3] & (np.arange(t - 3) != 2))   # the zero frequency band is perturbed
    assert np.array_equal(moved[:10, 3], signed[:10, 3])                # a column with one non-zero value is data
    if active is not None:
        assert np.array_equal(kept.view(np.uint32)[1], b0[1])           # inactive: -0.0 and NaN payloads kept
    ops.check_status()


def _raw(x0, x, g, out, batch, n_mels, t, eps=0.05, alpha=0.02, h="handle", cfg="cfg", active=None):
    c = _native.AdvConfig(eps, alpha, 1)
    handle = get_featurizer().handle if h == "handle" else h
    ptr = lambda v: v if v is None or isinstance(v, int) else v.data_ptr()          # noqa: E731
    return _native.lib().sir_adv_step(handle, ptr(x0), ptr(x), ptr(g), ptr(active), batch, n_mels, t,
                                      C.byref(c) if cfg == "cfg" else None, 7, ptr(out), _native.current_stream_ptr())


def test_every_refused_call_writes_nothing():
    bsz, t = 2, 24
    n = bsz * 64 * t
    x0 = torch.randn(n + 8, device=DEV)
    x = torch.randn(n + 8, device=DEV)
    g = torch.randn(n + 8, device=DEV)
    buf, out = _framed(n)
    act = torch.ones(4, dtype=torch.int32, device=DEV)
    einval, nan = _native.SIR_EINVAL, float("nan")
    before = [v.clone() for v in (x0, x, g)]
    refused = [
        _raw(x0, x, g, out, bsz, 64, t, h=None), _raw(None, x, g, out, bsz, 64, t), _raw(x0, x, g, None, bsz, 64, t),
        _raw(x0, x, g, out, bsz, 64, t, cfg=None),
        _raw(x0, x, g, out, 0, 64, t), _raw(x0, x, g, out, -1, 64, t), _raw(x0, x, g, out, bsz, 64, 0),
        _raw(x0, x, g, out, bsz, 0, t), _raw(x0, x, g, out, bsz, 65, t),
        _raw(x0, x, g, out, bsz, 64, t, eps=-0.1), _raw(x0, x, g, out, bsz, 64, t, eps=nan),
        _raw(x0, x, g, out, bsz, 64, t, alpha=-0.1), _raw(x0, x, g, out, bsz, 64, t, alpha=nan),
        _raw(x0, None, None, out, bsz, 64, t, eps=nan),
        _raw(x0, x, None, out, bsz, 64, t),                                            # x without g
        _raw(x0, None, g, out, bsz, 64, t),                                            # g without x
        _raw(x0, x, g, x0, bsz, 64, t), _raw(x0, x, g, g, bsz, 64, t),                 # out is x0 / g
        _raw(x0, x, g, x0.data_ptr() + 16, bsz, 64, t), _raw(x0, x, g, g.data_ptr() + 4 * (n - 1), bsz, 64, t),   # ... or overlaps
        _raw(x0, x, g, x.data_ptr() + 16, bsz, 64, t),                                 # out overlaps x without being x
        _raw(x0.data_ptr() + 2, x, g, out, bsz, 64, t), _raw(x0, x.data_ptr() + 1, g, out, bsz, 64, t),
        _raw(x0, x, g.data_ptr() + 2, out, bsz, 64, t), _raw(x0, x, g, out.data_ptr() + 2, bsz, 64, t),
        _raw(x0, x, g, out, bsz, 64, t, active=act.data_ptr() + 2),
    ]
    torch.cuda.synchronize()
    assert refused == [einval] * len(refused), refused
    assert (_bits(buf) == SENTINEL).all()
    for v, b in zip((x0, x, g), before):
        assert torch.equal(v, b)
    assert _native.lib().sir_last_error().startswith(b"sir_adv_step")
    # ... and the same arguments, accepted (alpha is not read on a random start)
    assert _raw(x0, x, g, out, bsz, 64, t) == 0 and _raw(x0, None, None, out, bsz, 64, t, alpha=nan) == 0
    assert _raw(x0, x, g, x, bsz, 64, t) == 0 and _raw(x0, x0, g, out, bsz, 64, t, active=act) == 0
    torch.cuda.synchronize()
    assert _frame_intact(buf, n)
    ops.check_status()


# ---- 2. the crafting pass leaves the module as it found it ------------------------------------------------------------
@pytest.mark.parametrize("frozen_bn", [(), (1,)])
def test_crafting_has_no_side_effects(sd, frozen_bn):
    bsz, t = 6, 24
    m = _model(sd, frozen_bn=frozen_bn, dropout=0.5)
    x = torch.randn(bsz, 64, t, generator=torch.Generator().manual_seed(3)).to(DEV)
    y = synth.synth_labels(bsz, 31, seed=4).to(DEV)
    train_ops.fused_cross_entropy(m(x), y).backward()                      # gradients in place, statistics tracked once
    grads = {n: p.grad for n, p in m.named_parameters()}
    grad_bits = {n: g.clone() for n, g in grads.items()}
    state = {k: v.clone() for k, v in m.state_dict().items()}
    flags = {n: mod.training for n, mod in m.named_modules()}
    step, epoch, last = train_ops.dropout_step(), ops._weights_epoch[0], m._sir_last_dropout
    adv = train_ops.Adversary(0.05, steps=3, random_start=True, prob=0.5, seed=1)
    x_adv = adv(m, x, lambda out: train_ops.fused_cross_entropy(out, y, label_smoothing=0.1))
    torch.cuda.synchronize()
    assert x_adv.shape == x.shape and not x_adv.requires_grad and x_adv.data_ptr() != x.data_ptr()
    assert 0 < (x_adv - x).abs().max().item() <= 0.05 * (1 + 1e-6) + 1e-6
    for k, v in m.state_dict().items():                                   # parameters, running statistics, num_batches_tracked
        assert torch.equal(v, state[k]), k
    for n, p in m.named_parameters():
        assert p.grad is grads[n] and torch.equal(p.grad, grad_bits[n]), n
    assert train_ops.dropout_step() == step and ops._weights_epoch[0] == epoch and m._sir_last_dropout == last
    assert {n: mod.training for n, mod in m.named_modules()} == flags
    ops.check_status()


# ---- 3. eps = 0 is the plain run ----------------------------------------------------------------------------------------
def _three_steps(sd, adversary, recipe):
    train_ops.set_dropout_step(1)
    m = _model(sd, dropout=0.5)
    opt = FusedAdam(m.parameters(), lr=1e-3, weight_decay=1e-4)
    gen = torch.Generator().manual_seed(21)
    loader = [(torch.randn(8, 64, 24, generator=gen), synth.synth_labels(8, 31, seed=30 + i)) for i in range(3)]
    criterion = torch.nn.CrossEntropyLoss(label_smoothing=0.1) if recipe else torch.nn.CrossEntropyLoss()
    mixup = train_ops.Mixup(0.4, seed=9) if recipe else None
    assert train_ops.adversary_of(m) is None
    train_ops.set_adversary(m, adversary)
    mean = tr.train_epoch(m, loader, opt, criterion, torch.device(DEV), None, mixup=mixup)
    return m, opt, mean, train_ops.dropout_step()


@pytest.mark.parametrize("recipe", [False, True])
def test_eps_zero_is_the_plain_run(sd, new_process, recipe):
    ma, oa, loss_a, step_a = _three_steps(sd, None, recipe)
    adv = train_ops.Adversary(eps=0.0, steps=2, random_start=True, seed=5)
    mb, ob, loss_b, step_b = _three_steps(sd, adv, recipe)
    assert loss_a == loss_b and step_a == step_b == 4
    for (k, a), b in zip(ma.state_dict().items(), mb.state_dict().values()):
        assert torch.equal(a, b), k
    sa, sb = oa.state[FusedAdam._key(0)], ob.state[FusedAdam._key(0)]
    assert sa["step"] == sb["step"] == 3
    for name in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(sa[name], sb[name]), name
    assert adv.rng.getstate() != train_ops.Adversary(0.0, seed=5).rng.getstate()         # it did draw: the passes ran
    ops.check_status()


# ---- 4. one step against the float64 oracle ----------------------------------------------------------------------------
def test_one_step_against_the_float64_oracle(sd):
    bsz, t, eps = 6, 24, 0.05
    x = torch.randn(bsz, 64, t, generator=torch.Generator().manual_seed(41))
    x[:, :, t - 8:] = 0.0
    y = synth.synth_labels(bsz, 31, seed=42)
    m = _model(sd, dropout=0.5)
    adv = train_ops.Adversary(eps=eps, steps=1, random_start=False)
    assert adv.alpha == eps
    yd = y.to(DEV)
    x_adv = adv(m, x.to(DEV), lambda out: train_ops.fused_cross_entropy(out, yd))
    torch.cuda.synchronize()
    zo, yo = ref.device_forward_values(m, sd, x, bsz, t)                   # the crafting forward's values (batch statistics)
    _, _, g_ref = ref.reference(sd, x, zo, yo, labels=y)
    g_ref = g_ref.numpy()
    x0 = x.numpy()
    want = adv_ref.adv_step(x0, x0, eps=eps, step=adv_ref.sign_step(g_ref, eps), keep_zero_columns=True)
    got = _bits(x_adv)
    live = np.broadcast_to(~adv_ref.zero_columns(x0), x0.shape)
    assert live[:, :, :t - 8].all() and not live[:, :, t - 8:].any()
    decided = np.abs(g_ref) > ref.GRAD_BOUND * np.sqrt((g_ref ** 2).mean())
    share = (live & ~decided).sum() / live.sum()
    wrong = (got != want.view(np.uint32)) & live & decided
    print(f"oracle step: {100 * share:.3f} % of the live elements below the gradient bound, {wrong.sum()} decided elements differ, "
          f"{((got != want.view(np.uint32)) & live).sum()} live elements differ in all")
    assert share <= 0.01
    assert wrong.sum() == 0
    assert (got[~live] == 0).all()                                         # the kept columns are exact +0.0
    ops.check_status()


# ---- 5. PGD loop consistency ------------------------------------------------------------------------------------------
def _eval_gradient(m, x, y):
    logits, leaf = explain._forward(m, x)
    with torch.enable_grad():
        loss = train_ops.fused_cross_entropy(logits, y)
    (g,) = torch.autograd.grad(loss, leaf)
    return g


@pytest.mark.parametrize("keep", [False, True])
def test_pgd_equals_a_host_loop_on_the_device_gradient(sd, keep):
    bsz, t, eps, steps, seed = 5, 24, 0.03, 3, 1234567890123
    x = torch.randn(bsz, 64, t, generator=torch.Generator().manual_seed(51))
    x[:, :, t - 5:] = 0.0
    y = synth.synth_labels(bsz, 31, seed=52).to(DEV)
    m = _model(sd).eval()
    got = explain.pgd(m, x.to(DEV), y, eps, steps=steps, random_start=True, seed=seed, keep_zero_columns=keep)
    alpha = adv_ref.default_alpha(eps, steps, True)
    x0 = x.numpy()
    cur = adv_ref.adv_step(x0, eps=eps, seed=seed, keep_zero_columns=keep)
    for _ in range(steps):
        g = _eval_gradient(m, torch.from_numpy(cur).to(DEV), y).cpu().numpy()
        cur = adv_ref.adv_step(x0, cur, g, eps, alpha, keep_zero_columns=keep)
    assert np.array_equal(_bits(got), cur.view(np.uint32))
    assert (np.abs(cur - x0) <= eps + 1e-6).all() and (cur[:, :, t - 5:] == 0).all() == keep
    ops.check_status()


def test_pgd_of_one_step_is_fgsm(sd):
    bsz, t, eps = 5, 24, 0.02
    x = torch.randn(bsz, 1, 64, t, generator=torch.Generator().manual_seed(53)).to(DEV)
    y = synth.synth_labels(bsz, 31, seed=54).to(DEV)
    m = _model(sd).eval()
    a, b = explain.pgd(m, x, y, eps, alpha=eps, steps=1, random_start=False), explain.fgsm(m, x, y, eps)
    assert a.shape == b.shape == x.shape and np.array_equal(_bits(a), _bits(b))
    assert np.array_equal(_bits(explain.pgd(m, x, y, eps, steps=1)), _bits(b))           # the default alpha of one step is eps
    ops.check_status()


# ---- 6. it ascends ----------------------------------------------------------------------------------------------------
def test_the_step_ascends_by_the_first_order_estimate(sd):
    bsz, t, eps = 8, 24, 0.01
    x = torch.randn(bsz, 64, t, generator=torch.Generator().manual_seed(61)).to(DEV)
    y = synth.synth_labels(bsz, 31, seed=62).to(DEV)
    m = _model(sd).eval()
    g = _eval_gradient(m, x, y)
    x_adv = explain.pgd(m, x, y, eps, steps=1)
    with torch.no_grad():
        ce, ce_adv = F.cross_entropy(m(x).double(), y).item(), F.cross_entropy(m(x_adv).double(), y).item()
    estimate = eps * g.double().abs().sum().item()
    print(f"ascent at eps {eps}: CE {ce:.6f} -> {ce_adv:.6f}, gain {ce_adv - ce:.3e} = {(ce_adv - ce) / estimate:.3f} of the first-order "
          f"estimate {estimate:.3e}")
    assert ce_adv - ce >= 0.5 * estimate > 0
    ops.check_status()


def test_robust_accuracy_counts_on_a_fitted_model(sd, new_process):
    bsz, t = 8, 24
    x = torch.randn(bsz, 64, t, generator=torch.Generator().manual_seed(63)).to(DEV)
    y = torch.arange(bsz, device=DEV) * 3
    m = _model(sd, dropout=0.0)
    finetune.freeze(m, {"bn_stats", "cnn"})                              # frozen statistics: the fit holds in eval semantics
    opt = FusedAdam(finetune.trainable_parameters(m), lr=1e-3, weight_decay=0.0)
    for _ in range(40):
        m.train()
        opt.zero_grad(set_to_none=True)
        train_ops.fused_cross_entropy(m(x), y).backward()
        opt.step()
    m.eval()
    assert int((m.predict(x)[1] == y).sum()) == bsz, "the fixture did not fit its batch"
    clean, adv = explain.robust_accuracy(m, x, y, 0.5, steps=5)
    assert clean.is_cuda and adv.is_cuda and clean.dtype == adv.dtype == torch.int64 and clean.dim() == adv.dim() == 0
    x_adv = explain.pgd(m, x, y, 0.5, steps=5)
    print(f"robust accuracy at eps 0.5, 5 steps: clean {int(clean)} / {bsz}, adversarial {int(adv)} / {bsz}")
    assert int(clean) == bsz and 0 <= int(adv) <= int(clean)
    assert int(adv) == int((m.predict(x_adv)[1] == y).sum())
    c0, a0 = explain.robust_accuracy(m, x, y, 0.0, steps=2)
    assert int(c0) == int(a0) == bsz                                     # radius 0: the clips themselves
    ops.check_status()


# ---- 7. resume ----------------------------------------------------------------------------------------------------------
CONFIG = {"lr": 1e-3, "weight_decay": 1e-2, "seed": 3, "batch_size": 8, "mixup": 0.2, "label_smoothing": 0.1,
          "adversarial": {"eps": 0.05, "steps": 2, "prob": 0.5}}
N_CLIPS, T = 32, 24


def _run_objects(sd):
    m = _model(sd, dropout=0.5)
    opt = FusedAdam(m.parameters(), lr=CONFIG["lr"], weight_decay=CONFIG["weight_decay"])
    a = tr.adversarial_options(CONFIG)
    adv = train_ops.Adversary(a["eps"], alpha=a["alpha"], steps=a["steps"], random_start=a["random_start"], prob=a["prob"],
                              seed=CONFIG["seed"] + 1231 * 0)
    return m, opt, train_ops.Mixup(CONFIG["mixup"], seed=CONFIG["seed"]), adv


def _epoch(store, epoch, m, opt, mixup, adv):
    batches = store.epoch_batches(CONFIG["batch_size"], shuffle=True, seed=CONFIG["seed"], epoch=epoch, augment_prob=0.5)
    criterion = torch.nn.CrossEntropyLoss(label_smoothing=CONFIG["label_smoothing"])
    train_ops.set_adversary(m, adv)
    return tr.train_epoch(m, batches, opt, criterion, torch.device(DEV), None, mixup=mixup)


def test_resumed_adversarial_run_is_bit_exact(sd, tmp_path, new_process):
    from sir_amd.feature_store import FeatureStore
    feats = synth.synth_features(N_CLIPS, T, seed=9).to(DEV)
    labels = synth.synth_labels(N_CLIPS, 31, seed=10).to(DEV)
    store = FeatureStore.from_tensors(feats, [T] * N_CLIPS, labels)
    steps_per_epoch = N_CLIPS // CONFIG["batch_size"]

    ma, oa, xa, aa = _run_objects(sd)
    _epoch(store, 0, ma, oa, xa, aa)
    loss_a = _epoch(store, 1, ma, oa, xa, aa)
    assert train_ops.dropout_step() == 1 + 2 * steps_per_epoch            # crafting drew no dropout key

    train_ops.set_dropout_step(1)
    mb, ob, xb, ab = _run_objects(sd)
    _epoch(store, 0, mb, ob, xb, ab)
    path = tmp_path / run_state.LATEST
    run_state.save_run_state(path, mb, ob, None, xb, epoch=0, config=CONFIG, adversary=ab)
    del mb, ob, xb, ab
    train_ops.set_dropout_step(1)
    mc, oc, xc, ac = _run_objects(synth.synth_state_dict(31, seed=1))      # other weights until the load
    with pytest.raises(ValueError, match="adversary"):
        run_state.load_run_state(path, mc, oc, None, xc, config=CONFIG)
    got = run_state.load_run_state(path, mc, oc, None, xc, config=CONFIG, adversary=ac)
    assert got["epoch"] == 0 and got["config_changed"] == [] and train_ops.dropout_step() == 1 + steps_per_epoch
    loss_c = _epoch(store, 1, mc, oc, xc, ac)

    assert loss_a == loss_c
    for (k, a), b in zip(ma.state_dict().items(), mc.state_dict().values()):
        assert torch.equal(a, b), k
    sa, sc = oa.state[FusedAdam._key(0)], oc.state[FusedAdam._key(0)]
    assert sa["step"] == sc["step"] == 2 * steps_per_epoch
    for name in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(sa[name], sc[name]), name
    assert aa.rng.getstate() == ac.rng.getstate()
    ops.check_status()


# ---- 8. through train(): the YAML key, robust validation, checkpoint and resume -------------------------------------------
def test_train_entry_point_with_the_adversarial_key(tmp_path, new_process, capsys):
    import json
    import types

    import pandas as pd

    from sir_amd.scripts import precompute_features as pf
    from test_pipeline_gpu import LABELS, _make_corpus

    rows = _make_corpus(str(tmp_path / "wav"))
    csvs = {}
    for split, sl in (("train", slice(0, 16)), ("valid", slice(16, 20))):
        p = tmp_path / f"{split}_data.csv"
        pd.DataFrame(rows[sl]).to_csv(p, index=False)
        csvs[split] = str(p)
        pf.precompute_dataset_features(str(p), str(tmp_path / "cache"))
    lm = tmp_path / "label_map.json"
    lm.write_text(json.dumps({l: i for i, l in enumerate(sorted(LABELS))}))
    args = types.SimpleNamespace(train_csv=csvs["train"], val_csv=csvs["valid"], label_map=str(lm))
    cfg = {"batch_size": 8, "num_workers": 0, "num_labels": 31, "lr": 1e-3, "weight_decay": 1e-2, "early_stop_patience": 5,
           "augment_prob": 0.7, "cache_dir": str(tmp_path / "cache"), "use_feature_cache": True, "seed": 2, "mixup": 0.2,
           "label_smoothing": 0.1, "checkpoint_every_epoch": True,
           "adversarial": {"eps": 0.02, "steps": 2, "prob": 0.5, "validate": True}}

    def run(save_dir, **kw):
        torch.manual_seed(1234)
        train_ops.set_dropout_step(1)
        return tr.train(args, dict(cfg, save_path=str(tmp_path / save_dir), **kw))

    with pytest.raises(ValueError, match="unknown keys"):                  # refused before anything is built
        tr.train(args, dict(cfg, adversarial={"eps": 0.02, "radius": 1}))
    run("resumed", epochs=1)
    out = capsys.readouterr().out
    assert "Robust val accuracy (eps 0.02, 2 steps):" in out
    latest = tmp_path / "resumed" / run_state.LATEST
    saved = torch.load(latest, weights_only=False)
    assert saved["per_rank"][0]["adversary_rng"] is not None and saved["config"]["adversarial"] == cfg["adversarial"]
    with pytest.raises(ValueError, match="adversary"):                     # the resuming run must have one too
        run("resumed", epochs=2, resume=True, adversarial=None)
    run("resumed", epochs=2, resume=True)
    run("straight", epochs=2)
    a = torch.load(latest, weights_only=False)
    b = torch.load(tmp_path / "straight" / run_state.LATEST, weights_only=False)
    assert a["epoch"] == b["epoch"] == 1 and a["per_rank"] == b["per_rank"]
    for k, v in a["model_state_dict"].items():
        assert torch.equal(v, b["model_state_dict"][k]), k
    sa, sb = a["optimizer_state_dict"]["state"]["_sir_group_0"], b["optimizer_state_dict"]["state"]["_sir_group_0"]
    assert sa["step"] == sb["step"] == 4
    for name in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(sa[name], sb[name]), name
    ops.check_status()
