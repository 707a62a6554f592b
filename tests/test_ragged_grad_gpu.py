"""GPU: the ragged differentiable step (``sir_model_train_fwd_ragged`` / ``sir_model_train_bwd_ragged``, ``model(x, lengths=...)`` with
frozen BatchNorm statistics, ``sir_amd.explain.*_ragged``) against the per-clip float64 reference of tests/ragged_grad_ref.py.

Reference: per-clip ``oracle.model_ref.forward(sd64, x[b:b+1, :, :frames[b]], train=False, dropout_mask=..., z_override=...,
y_override=...)`` under autograd, loss = mean CE over the rows, evaluated at the device's forward values sliced to each clip's widths
(``input_grad_ref.device_forward_values``); the dropout mask is the dense step's, checked against workspace slots 8 / 9.
Bounds: gradients ``max |a - ref| <= 2e-3 * rms(ref)``, logits 2e-5, loss 1e-5; ``attention.bias`` (reference maximum <= 1e-7) skipped.
Every parity test prints its measured ratios under ``-s``.
"""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import cases
import input_grad_ref
import ragged_grad_ref as rg
from sir_amd import _native, explain, ops, synth, train_ops
from sir_amd.featurizer import get_featurizer

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES10 = rg.CASE_FRAMES
FRAMES33 = [8, 9, 15, 16, 17, 23, 31, 32, 33, 47, 63, 64, 94, 95, 120, 199, 200, 8, 200, 94, 13, 77, 150, 40, 24, 25, 100, 101, 55, 8,
            200, 12, 187]                                # (tests/test_ragged_infer_gpu.py::FRAMES)


def _arranged33():
    """FRAMES33 with a first group of 16 that holds only clips shorter than the batch's longest (S_b <= 18 of S = 25): that
    cluster of the forward recurrence runs fewer steps than S.  The last group holds one clip: partly empty."""
    short = [i for i, f in enumerate(FRAMES33) if f < 150][:16]
    order = short + [i for i in range(33) if i not in short]
    frames = [FRAMES33[i] for i in order]
    assert sorted(frames) == sorted(FRAMES33) and max(frames[:16]) < 150 and max(frames) == 200
    return frames


@pytest.fixture(scope="module")
def sd():
    return synth.synth_state_dict(31, seed=0)


@pytest.fixture(scope="module")
def case10():
    x = cases.varied_features(10, 40, seed=21).float()
    return x, synth.synth_labels(10, 31, seed=22)


def _nan_tails(x, frames):
    x = x.clone()
    for b, f in enumerate(frames):
        x[b, :, f:] = float("nan")
    return x


def _equal_out(a, b):
    assert torch.equal(a["logits"], b["logits"]) and torch.equal(a["loss"], b["loss"]) and torch.equal(a["dx"], b["dx"])
    for k in a["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), k


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_case10_vs_per_clip_reference(sd, case10, p):
    """1. + 2.: t_frames 40, batch 10, S_b = 1, an odd width at every stage, a full-width clip; all 29 gradients, dx, logits, loss;
    dx exactly zero behind every clip.  Then the same step on a workspace filled with 0xFF and NaN behind every clip: finite and
    bit-identical (nothing behind a clip's widths is read as data).  A rerun of the whole step is bit-identical.
    Measured on MI355X (worst gradient ratio / dx / logits / loss): dropout 0: 1.0e-5 (conv3.weight) / 4.8e-6 / 7.1e-8 / 1.1e-9;
    dropout 0.5: 1.5e-5 (gru.weight_ih_l0_reverse) / 5.6e-6 / 1.0e-7 / 4.9e-8."""
    x, y = case10
    m = rg.frozen_model(sd, p)
    train_ops.set_dropout_step(11)
    out = rg.ragged_step(m, x, FRAMES10, y)
    ref = rg.reference_for(m, sd, x, FRAMES10, y, p)
    rg.check_against(out, ref, FRAMES10, f"case10 p={p}")
    train_ops.set_dropout_step(11)
    out_nan = rg.ragged_step(m, _nan_tails(x, FRAMES10), FRAMES10, y, fill=0xFF)
    assert all(torch.isfinite(v).all() for v in [out_nan["logits"], out_nan["loss"], out_nan["dx"]] + list(out_nan["grads"].values()))
    _equal_out(out, out_nan)
    train_ops.set_dropout_step(11)
    _equal_out(out, rg.ragged_step(m, x, torch.tensor(FRAMES10, dtype=torch.int32, device=DEV), y))     # rerun, device lengths
    ops.check_status()


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_case33_vs_per_clip_reference(sd, p):
    """3.: t_frames 200, batch 33 (two full GRU groups + one clip), one group of 16 holding only clips shorter than the longest.  With
    dropout 0 the forward logits also agree with ``model.eval()(x, lengths=...)`` within 2e-5.
    Measured on MI355X: dropout 0: 1.2e-5 (dx) / 1.2e-5 / 1.1e-7 / 2.0e-7, 1.2e-7 from the eval call; dropout 0.5: 1.5e-5 (dx) / 1.5e-5 /
    1.5e-7 / 4.8e-8."""
    frames = _arranged33()
    x = cases.varied_features(33, 200, seed=11).float()
    y = synth.synth_labels(33, 31, seed=23)
    m = rg.frozen_model(sd, p)
    out = rg.ragged_step(m, _nan_tails(x, frames), frames, y, fill=0xFF)
    ref = rg.reference_for(m, sd, x, frames, y, p)
    rg.check_against(out, ref, frames, f"case33 p={p}")
    if p == 0.0:
        m.eval()
        with torch.no_grad():
            lg = m(x.to(DEV), lengths=frames).cpu()
        d = (lg - out["logits"]).abs().max().item()
        print(f"case33: training-path logits vs model.eval()(x, lengths): {d:.2e}")
        assert d <= rg.LOGIT_BOUND
    ops.check_status()


@pytest.mark.parametrize("t,bsz", [(24, 5), (200, 3)])
def test_full_length_clips_agree_with_the_dense_frozen_step(sd, t, bsz):
    """4.: all frames == t_frames: the dense frozen step (sir_model_train_bwd_x, all frozen) within the gradient bound.  Whether the two
    are bit-identical is printed, not required."""
    x = cases.varied_features(bsz, t, seed=31).float()
    y = synth.synth_labels(bsz, 31, seed=32)
    m = rg.frozen_model(sd, 0.5)
    train_ops.set_dropout_step(7)
    rag = rg.ragged_step(m, x, [t] * bsz, y)
    train_ops.set_dropout_step(7)
    xd = x.to(DEV).requires_grad_(True)
    for q in m.parameters():
        q.grad = None
    logits = m(xd)
    loss = train_ops.fused_cross_entropy(logits, y.to(DEV))
    loss.backward()
    dense = {n: q.grad.cpu() for n, q in m.named_parameters()}
    r = {k: rg.ratio(rag["grads"][k], v) for k, v in dense.items() if v.abs().max() > rg.SKIP_BELOW}
    r["dx"] = rg.ratio(rag["dx"], xd.grad.cpu())
    same = all(torch.equal(rag["grads"][k], v) for k, v in dense.items()) and torch.equal(rag["dx"], xd.grad.cpu()) and \
        torch.equal(rag["logits"], logits.detach().cpu())
    print(f"full-length t={t}: bit-identical to the dense frozen step: {same}; worst ratio {max(r.values()):.2e}")
    assert (rag["logits"] - logits.detach().cpu()).abs().max() <= rg.LOGIT_BOUND
    assert max(r.values()) <= rg.GRAD_BOUND, r
    ops.check_status()


# ---- the C calls ------------------------------------------------------------------------------------------------------------------
def _cfg(frozen=(1, 1, 1)):
    cfg = _native.TrainConfig()
    for i in range(3):
        cfg.bn_frozen[i] = frozen[i]
    return cfg


class _CStep:
    """sir_model_train_fwd_ragged / _bwd_ragged on the module's own training workspace and gradient buffer."""

    def __init__(self, m, x, frames, p=0.0, seed=99):
        self.lib, self.h = _native.lib(), get_featurizer().handle
        self.m, self.x, self.p, self.seed = m, x.to(DEV).contiguous(), p, seed
        self.frames = torch.tensor(list(frames), dtype=torch.int32, device=DEV)
        self.bsz, self.t = x.shape[0], x.shape[-1]
        self.w, self.keep = ops.cached_weights(m)
        self.st = train_ops._train_state(m)
        self.ws = self.st["ws"].get(self.lib.sir_model_workspace_bytes(self.h, self.bsz, self.t, 1), self.x.device)
        self.rm, self.rv = train_ops._bn_ptr_arrays(m)

    def fwd(self, logits, cfg=None, frames=None):
        frames = self.frames if frames is None else frames
        return self.lib.sir_model_train_fwd_ragged(self.h, C.byref(self.w), self.rm, self.rv, self.x.data_ptr(), frames.data_ptr(), self.bsz,
                                                   self.t, self.p, self.seed, C.byref(cfg) if cfg is not None else None, logits.data_ptr(),
                                                   self.ws.data_ptr(), self.ws.numel(), _native.current_stream_ptr())

    def bwd(self, dlogits, parts, cfg=None, frames=None, dx=None):
        frames = self.frames if frames is None else frames
        grads = self.st["grads"]
        rcs = [self.lib.sir_model_train_bwd_ragged(self.h, C.byref(self.w), self.x.data_ptr(), frames.data_ptr(), dlogits.data_ptr(), self.bsz,
                                                   self.t, self.p, self.seed, C.byref(cfg) if cfg is not None else None,
                                                   C.byref(grads.struct), dx.data_ptr() if dx is not None else None, self.ws.data_ptr(),
                                                   self.ws.numel(), part, _native.current_stream_ptr()) for part in parts]
        torch.cuda.synchronize()
        return rcs, grads.flat.clone()


def test_pruning_and_halves(sd, case10):
    """5.: only fc and attention wanted -> their gradients bit-identical to the full call's and no conv backward scope runs;
    SIR_BWD_HEAD_GRU then SIR_BWD_CNN bit-identical to SIR_BWD_ALL (the one-stream form, under the profile, agrees too)."""
    x, y = case10
    m = rg.frozen_model(sd, 0.5)
    train_ops.set_dropout_step(13)
    full = rg.ragged_step(m, x, FRAMES10, y)
    one = {}

    def full_again():
        train_ops.set_dropout_step(13)
        one.update(rg.ragged_step(m, x, FRAMES10, y))

    counts, _ = input_grad_ref.launch_counts(full_again)     # the whole step in the one-stream form: the same bits
    _equal_out(full, one)
    assert all(counts[k] > 0 for k in ("bwd_head", "bwd_gru_l1", "bwd_gru_l0", "bwd_bn3", "bwd_bn2", "bwd_conv1", "bwd_conv1_dgrad"))
    mp = rg.frozen_model(sd, 0.5)
    for n, q in mp.named_parameters():
        q.requires_grad_(n.startswith(("fc.", "attention.")))
    xd = x.to(DEV)
    out = {}

    def pruned():
        train_ops.set_dropout_step(13)
        for q in mp.parameters():
            q.grad = None
        loss = train_ops.fused_cross_entropy(mp(xd, lengths=FRAMES10), y.to(DEV))
        loss.backward()
        out.update({n: q.grad.cpu() for n, q in mp.named_parameters() if q.grad is not None})

    pruned()
    assert sorted(out) == ["attention.bias", "attention.weight", "fc.bias", "fc.weight"]
    for n, g in out.items():
        assert torch.equal(g, full["grads"][n]), n
    counts, _ = input_grad_ref.launch_counts(pruned)
    conv_ids = ("bwd_bn3", "bwd_conv3_wgrad", "bwd_conv3_dgrad", "bwd_bn2", "bwd_conv2_wgrad", "bwd_conv2_dgrad", "bwd_conv1", "bwd_conv1_dgrad",
                "bwd_gru_l1", "bwd_gru_l0")
    print("fc + attention only, launches:", {k: counts[k] for k in conv_ids + ("bwd_head",)})
    assert counts["bwd_head"] > 0 and all(counts[k] == 0 for k in conv_ids)
    for n, g in out.items():                             # (the profiled run is the one-stream form)
        assert torch.equal(g, full["grads"][n]), n
    # the halves, through the C calls
    cs = _CStep(m, x, FRAMES10, p=0.5, seed=1234)
    logits = torch.empty(10, 31, device=DEV)
    assert cs.fwd(logits, _cfg()) == _native.SIR_OK
    dlogits = (torch.softmax(logits, 1) - torch.nn.functional.one_hot(y.to(DEV), 31)) / 10
    dx_all, dx_two = torch.empty_like(cs.x), torch.empty_like(cs.x)
    rcs, g_all = cs.bwd(dlogits, [_native.BWD_ALL], _cfg(), dx=dx_all)
    assert rcs == [_native.SIR_OK]
    rcs, g_two = cs.bwd(dlogits, [_native.BWD_HEAD_GRU, _native.BWD_CNN], _cfg(), dx=dx_two)
    assert rcs == [_native.SIR_OK, _native.SIR_OK]
    assert torch.equal(g_all, g_two) and torch.equal(dx_all, dx_two) and g_all.abs().max() > 0 and dx_all.abs().max() > 0
    ops.check_status()


def test_refusals_write_nothing_and_bad_lengths_stay_in_their_rows(sd, case10):
    """6.: a cfg with a live block and cfg == NULL are SIR_EUNSUPPORTED, sentinel logits untouched.  Device frames holding 7 and
    t_frames + 1: NaN logits in those rows only, SIR_EINVAL from sir_check_status, the other rows' logits and dx bit-identical to the
    call in which those rows hold valid lengths (rows are independent under frozen statistics), the bad rows' dx zero."""
    x, y = case10
    m = rg.frozen_model(sd, 0.0)
    cs = _CStep(m, x, FRAMES10)
    sentinel = torch.full((10, 31), 12345.0, device=DEV)
    for cfg in (None, _cfg((1, 0, 1)), _cfg((0, 0, 0))):
        logits = sentinel.clone()
        assert cs.fwd(logits, cfg) == _native.SIR_EUNSUPPORTED
        msg = cs.lib.sir_last_error().decode()
        assert "lengths" in msg and "frozen" in msg, msg
        rcs, _ = cs.bwd(sentinel, [_native.BWD_ALL], cfg)
        assert rcs == [_native.SIR_EUNSUPPORTED]
        torch.cuda.synchronize()
        assert torch.equal(logits, sentinel)
    ops.check_status()
    # good call
    logits = torch.empty(10, 31, device=DEV)
    assert cs.fwd(logits, _cfg()) == _native.SIR_OK
    seed = torch.zeros(10, 31, device=DEV)
    seed[torch.arange(10), y.to(DEV)] = 1.0 / 16
    dx_good = torch.empty_like(cs.x)
    empty = _native.ModelGrads()

    def data_bwd(frames, dl, dx):
        rc = cs.lib.sir_model_train_bwd_ragged(cs.h, C.byref(cs.w), cs.x.data_ptr(), frames.data_ptr(), dl.data_ptr(), 10, 40, 0.0, cs.seed,
                                               C.byref(_cfg()), C.byref(empty), dx.data_ptr(), cs.ws.data_ptr(), cs.ws.numel(), _native.BWD_ALL,
                                               _native.current_stream_ptr())
        assert rc == _native.SIR_OK
        torch.cuda.synchronize()

    data_bwd(cs.frames, seed, dx_good)
    ops.check_status()
    bad = cs.frames.clone()
    bad[2], bad[7] = 7, 41
    lg_bad = torch.empty(10, 31, device=DEV)
    assert cs.fwd(lg_bad, _cfg(), frames=bad) == _native.SIR_OK
    with pytest.raises(_native.SirError):
        ops.check_status()
    dl = seed.clone()
    dl[2], dl[7] = float("nan"), 3.0                     # whatever the bad rows' dlogits hold
    dx_bad = torch.full_like(cs.x, 777.0)
    data_bwd(bad, dl, dx_bad)
    ok = [b for b in range(10) if b not in (2, 7)]
    assert lg_bad[[2, 7]].isnan().all() and not lg_bad[ok].isnan().any()
    assert torch.equal(lg_bad[ok], logits[ok]) and torch.equal(dx_bad[ok], dx_good[ok])
    assert torch.equal(dx_bad[[2, 7]], torch.zeros_like(dx_bad[[2, 7]]))
    ops.check_status()                                   # (the backward raises nothing of its own)


def test_input_gradient_ragged_is_input_gradient_clip_by_clip(sd):
    """7.: batch 5; each row against ``explain.input_gradient`` on that clip alone, sliced to its length.  Bit-identical is expected
    (as for ragged inference); otherwise within the gradient bound, the figure printed."""
    frames = [40, 9, 23, 16, 31]
    x = cases.varied_features(5, 40, seed=41).float()
    m = rg.frozen_model(sd, 0.5).eval()
    xn = _nan_tails(x, frames).to(DEV)
    target = torch.tensor([3, 0, 30, 7, 7])
    lg, dx = explain.input_gradient_ragged(m, xn, frames, target)
    assert torch.equal(dx.isnan(), torch.zeros_like(dx, dtype=torch.bool))
    worst, same = 0.0, True
    for b, f in enumerate(frames):
        lg1, dx1 = explain.input_gradient(m, x[b:b + 1, :, :f].contiguous().to(DEV), target[b:b + 1])
        same = same and torch.equal(dx[b, :, :f], dx1[0]) and torch.equal(lg[b], lg1[0])
        worst = max(worst, rg.ratio(dx[b, :, :f], dx1[0]))
        assert (lg[b] - lg1[0]).abs().max() <= rg.LOGIT_BOUND
        assert torch.equal(dx[b, :, f:], torch.zeros_like(dx[b, :, f:]))
    print(f"input_gradient_ragged vs clip by clip: bit-identical {same}, worst ratio {worst:.2e}")
    assert worst <= rg.GRAD_BOUND
    sal = explain.saliency_ragged(m, xn, frames, target)
    assert sal.shape == (5, 64, 40) and not sal.isnan().any() and torch.equal(sal, (dx * x.to(DEV)).abs())     # (x: the clean copy)
    adv = explain.fgsm_ragged(m, xn, [1, 2, 3, 4, 5], 0.01, frames)
    for b, f in enumerate(frames):
        assert adv[b, :, f:].isnan().all()               # as they came
        assert ((adv[b, :, :f] - xn[b, :, :f]).abs() <= 0.01 + 1e-5).all() and (adv[b, :, :f] != xn[b, :, :f]).any()
    with pytest.raises(ValueError, match="lengths"):
        explain.input_gradient(m, xn, lengths=frames)
    ops.check_status()


_CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}, {golden!r}]
import torch
import cases
import ragged_grad_ref as rg
from sir_amd import ops, synth, train_ops
sd = synth.synth_state_dict(31, seed=0)
x = cases.varied_features(10, 40, seed=21).float()
y = synth.synth_labels(10, 31, seed=22)
m = rg.frozen_model(sd, 0.5)
out = rg.ragged_step(m, x, rg.CASE_FRAMES, y, fill=0xFF)
rg.check_against(out, rg.reference_for(m, sd, x, rg.CASE_FRAMES, y, 0.5), rg.CASE_FRAMES, "fallback")
ops.check_status()
print("RAGGED-GRAD-FALLBACK-OK")
"""


def test_fallback_conv_route(tmp_path):
    """8.: case 1 with dropout 0.5 on the first-generation / direct conv kernels and the nine-tap weight gradient (SIR_CONV_FALLBACK=2
    is read once per process: a fresh child under its own time limit, as tests/test_conv_fallback_gpu.py drives it)."""
    script = tmp_path / "ragged_grad_fallback.py"
    script.write_text(_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), golden=os.path.join(ROOT, "tests", "golden")))
    env = dict(os.environ, SIR_CONV_FALLBACK="2")
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, str(script)], capture_output=True, text=True, env=env, cwd=ROOT)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "RAGGED-GRAD-FALLBACK-OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
