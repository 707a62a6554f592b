"""Fine-tuning semantics of the training step on the GPU: frozen BatchNorm statistics (``bnK.eval()`` inside ``model.train()``),
``gru.eval()``, and a backward that stops where the trainable parameters stop (``sir_model_train_fwd_cfg`` / ``_bwd_cfg``).

Reference: ``tests/golden/finetune_golden.npz`` -- the reference's own ``CNNAudioGRU`` on CPU in fp32 driven with the torch idiom
(``tests/golden/make_finetune_golden.py``).  Tolerances are those of ``test_train_gpu.py::test_train_step_matches_reference_golden``:
logits 2e-5, loss 1e-5, gradients 2e-3 of the tensor's rms, the conv / bn gradients 2e-2 because the golden inputs have pooling
windows whose two largest values lie within 1e-6 (``*/near_ties`` in the golden file: 1-2 windows per block).
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cases
import finetune_ref
from sir_amd import _native, finetune, synth, train_ops
from sir_amd.featurizer import get_featurizer
from sir_amd.models.models import CNNAudioGRU
from sir_amd.optim import FusedAdam

pytestmark = pytest.mark.gpu
DEV = "cuda"

CNN = ("conv", "bn")
BWD_IDS = ("bwd_head", "bwd_gru_l1", "bwd_gru_dw_l1", "bwd_gru_dx_l1", "bwd_gru_l0", "bwd_gru_dw_l0", "bwd_gru_dx_l0", "bwd_bn3",
           "bwd_conv3_wgrad", "bwd_conv3_dgrad", "bwd_bn2", "bwd_conv2_wgrad", "bwd_conv2_dgrad", "bwd_conv1")
BELOW_GRU = ("bwd_gru_dx_l0", "bwd_bn3", "bwd_conv3_wgrad", "bwd_conv3_dgrad", "bwd_bn2", "bwd_conv2_wgrad", "bwd_conv2_dgrad", "bwd_conv1")


@pytest.fixture(scope="module")
def sd():
    return synth.synth_state_dict(31, seed=0)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(cases.GOLDEN_DIR, "finetune_golden.npz"))


def _model(sd, frozen_bn=(), dropout=0.0):
    m = CNNAudioGRU(31)
    m.load_state_dict(sd)
    m = m.to(DEV).train()
    m.gru.dropout = dropout
    for i in frozen_bn:
        getattr(m, f"bn{i}").eval()
    return m


def _step(m, x, y):
    m.zero_grad(set_to_none=True)
    logits = m(x)
    loss = train_ops.fused_cross_entropy(logits, y)
    loss.backward()
    torch.cuda.synchronize()
    return logits, loss


def _check_against_golden(m, logits, loss, golden, case):
    print(case, "loss", loss.item(), "golden", float(golden[f"{case}/loss"]))
    assert abs(loss.item() - float(golden[f"{case}/loss"])) < 1e-5
    np.testing.assert_allclose(logits.detach().cpu().numpy(), golden[f"{case}/logits"], rtol=0, atol=2e-5)
    errs = {}
    for name, p in m.named_parameters():
        g = p.grad.detach().cpu().flatten()
        idx = cases.sample_indices(name, g.numel())
        norm = float(golden[f"{case}/grad_norm/{name}"])
        rms = norm / np.sqrt(g.numel())
        errs[name] = (np.abs(g[idx].numpy() - golden[f"{case}/grad_samp/{name}"]).max() / (rms + 1e-30),
                      abs(g.double().norm().item() - norm) / (norm + 1e-30))
    print(case, "grad errors (max sampled |a-b| / rms, norm rel):", {k: f"{a:.1e}/{b:.1e}" for k, (a, b) in errs.items()})
    for name, p in m.named_parameters():
        g = p.grad.detach().cpu().flatten()
        idx = cases.sample_indices(name, g.numel())
        norm = float(golden[f"{case}/grad_norm/{name}"])
        rms = norm / np.sqrt(g.numel())
        tol = 2e-2 if name.startswith(CNN) else 2e-3      # pooling near-ties of the golden inputs, see the module docstring
        assert np.abs(g[idx].numpy() - golden[f"{case}/grad_samp/{name}"]).max() <= tol * rms + 1e-7, name
        assert abs(g.double().norm().item() - norm) <= 0.5 * tol * norm + 1e-7, name


def test_all_three_bn_frozen_matches_reference(sd, golden):
    """bn1..3.eval() inside model.train(): loss, logits and all 29 gradients follow the reference; the running statistics and
    num_batches_tracked are bit-unchanged (and equal the reference's, which did not move either)."""
    inp = cases.model_inputs()
    m = _model(sd, frozen_bn=(1, 2, 3))
    before = {k: v.clone() for k, v in m.state_dict().items() if "running" in k or "tracked" in k}
    logits, loss = _step(m, inp["x_train8"].to(DEV), inp["y_train8"].to(DEV))
    _check_against_golden(m, logits, loss, golden, "frozen")
    for k, v in before.items():
        assert torch.equal(m.state_dict()[k], v), k
    for i in (1, 2, 3):
        assert torch.equal(getattr(m, f"bn{i}").running_mean.cpu(), torch.from_numpy(golden[f"frozen/bn{i}.running_mean"]))
        assert int(getattr(m, f"bn{i}").num_batches_tracked) == int(golden[f"frozen/bn{i}.num_batches_tracked"]) == 0


def _device_forward_values(m, sd, x, bsz, t):
    """What the device's ReLU / max-pool compared, rebuilt on the host as ``test_train_gpu.py`` does: z2 / z3 from the workspace, z1
    (never stored) as conv1's chain of nine fmas, y = fma(z, scale, shift) with the device's folded scale / shift; NCHW."""
    lib = _native.lib()
    offs = (C.c_size_t * 40)()
    assert lib.sir_model_train_workspace_offsets(get_featurizer().handle, bsz, t, offs, 40) > 0
    ws = m._sir_train["ws"].buf
    wp1, wp2 = t // 2, t // 4
    z2 = ws[offs[1]: offs[1] + 4 * bsz * 32 * wp1 * 64].view(torch.float32).view(bsz, 32, wp1, 64).cpu()
    z3 = ws[offs[3]: offs[3] + 4 * bsz * 16 * wp2 * 128].view(torch.float32).view(bsz, 16, wp2, 128).cpu()
    bn = ws[offs[12]: offs[12] + 4 * 448].view(torch.float32).cpu()
    scale, shift = bn[:224], bn[224:448]
    fma32 = lambda a, b, c: (a.double() * b.double() + c.double()).float()
    xp = torch.nn.functional.pad(x.float(), (1, 1, 1, 1))
    w1 = sd["conv1.weight"].float().view(32, 9)
    z1 = torch.zeros(bsz, 32, 64, t)
    for ky in range(3):
        for kx in range(3):
            z1 = fma32(xp[:, None, ky:ky + 64, kx:kx + t], w1[None, :, ky * 3 + kx, None, None], z1)
    z = {1: z1, 2: z2.permute(0, 3, 1, 2), 3: z3.permute(0, 3, 1, 2)}
    y = {i: fma32(z[i], scale[o:o + c][None, :, None, None], shift[o:o + c][None, :, None, None])
         for i, o, c in ((1, 0, 32), (2, 32, 64), (3, 96, 128))}
    return z, y


def test_all_three_bn_frozen_at_bench_batch_256_vs_reference(sd):
    """B = 256, T = 200 with bn1..3.eval(): the shapes where the frozen dz form's grid stride, the GRU-layout reads and the slab plans
    differ from the 8-clip golden batch.  Reference: ``tests/finetune_ref.py`` (pinned to the reference's module by the golden
    file) in float64, differentiated at the device's ReLU / pool decisions (z / y override), as
    ``test_train_gpu.py::test_training_step_at_bench_batch_256_vs_oracle`` does and with its bounds: loss 2e-5, logits 5e-5, every
    gradient 2e-3 of its rms, norms 1e-3.  Running statistics and num_batches_tracked bit-unchanged."""
    bsz, t = 256, 200
    x = cases.varied_features(bsz, t, seed=256)
    y = synth.synth_labels(bsz, 31, seed=257)
    m = _model(sd, frozen_bn=(1, 2, 3))
    before = {k: v.clone() for k, v in m.state_dict().items() if "running" in k or "tracked" in k}
    logits, loss = _step(m, x.to(DEV), y.to(DEV))
    zo, yo = _device_forward_values(m, sd, x, bsz, t)
    d = lambda v: v.double() if torch.is_tensor(v) and v.is_floating_point() else v
    ref_loss, ref_grads, _, ref_logits = finetune_ref.loss_and_grads(
        {k: d(v) for k, v in sd.items()}, d(x), y, bn_frozen=(True, True, True),
        z_override={k: d(v) for k, v in zo.items()}, y_override={k: d(v) for k, v in yo.items()})
    del zo, yo
    print("B=256 frozen: loss", loss.item(), "ref", ref_loss.item(),
          "logits max err", (logits.detach().cpu().double() - ref_logits).abs().max().item())
    gerr = {}
    for name, p in m.named_parameters():
        r = ref_grads[name]
        diff = (p.grad.cpu().double() - r).abs().max().item()
        gerr[name] = diff if r.abs().max() <= 1e-7 else diff / (r.pow(2).mean().sqrt().item() + 1e-30)
    print("B=256 frozen-BN grad errors:", {k: f"{e:.1e}" for k, e in gerr.items()})
    assert abs(loss.item() - ref_loss.item()) < 2e-5
    assert (logits.detach().cpu().double() - ref_logits).abs().max() < 5e-5
    for k, e in gerr.items():
        assert e < 2e-3 or k == "attention.bias", (k, e)      # (attention.bias: true gradient 0 -- softmax shift invariance)
    for name, p in m.named_parameters():
        rn = ref_grads[name].norm().item()
        assert abs(p.grad.double().norm().item() - rn) <= 1e-3 * rn + 1e-7, name
    for k, v in before.items():
        assert torch.equal(m.state_dict()[k], v), k


def test_mixed_bn1_frozen_bn2_bn3_live_matches_reference(sd, golden):
    inp = cases.model_inputs()
    m = _model(sd, frozen_bn=(1,))
    rm1, rv1 = m.bn1.running_mean.clone(), m.bn1.running_var.clone()
    logits, loss = _step(m, inp["x_train8"].to(DEV), inp["y_train8"].to(DEV))
    _check_against_golden(m, logits, loss, golden, "mixed")
    assert torch.equal(m.bn1.running_mean, rm1) and torch.equal(m.bn1.running_var, rv1) and int(m.bn1.num_batches_tracked) == 0
    for i in (2, 3):
        bn = getattr(m, f"bn{i}")
        np.testing.assert_allclose(bn.running_mean.cpu().numpy(), golden[f"mixed/bn{i}.running_mean"], rtol=1e-4, atol=1e-6)
        np.testing.assert_allclose(bn.running_var.cpu().numpy(), golden[f"mixed/bn{i}.running_var"], rtol=1e-4, atol=1e-6)
        assert int(bn.num_batches_tracked) == int(golden[f"mixed/bn{i}.num_batches_tracked"]) == 1


def test_gru_eval_inside_train_turns_dropout_off(sd):
    inp = cases.model_inputs()
    x, y = inp["x_train8"].to(DEV), inp["y_train8"].to(DEV)
    m0 = _model(sd, dropout=0.0)
    lg0, loss0 = _step(m0, x, y)
    m1 = _model(sd, dropout=0.5)
    m1.gru.eval()
    lg1, loss1 = _step(m1, x, y)
    assert m1._sir_last_dropout[1] == 0.0
    assert torch.equal(lg0, lg1) and torch.equal(loss0, loss1)
    for (n, p), (_, q) in zip(m0.named_parameters(), m1.named_parameters()):
        assert torch.equal(p.grad, q.grad), n


def _freeze_names(m, pred):
    for n, p in m.named_parameters():
        p.requires_grad_(not pred(n))


PRUNE_SETS = {
    # name: (frozen-parameter predicate, BatchNorm blocks in eval(), kernel ids that must not be launched)
    "head_only": (lambda n: not n.startswith(("fc.", "attention.")), (), tuple(k for k in BWD_IDS if k != "bwd_head")),
    "gru_and_head": (lambda n: n.startswith(CNN), (), BELOW_GRU),
    "cnn_and_bn_frozen": (lambda n: n.startswith(CNN), (1, 2, 3), BELOW_GRU),
    "conv2_weight": (lambda n: n == "conv2.weight", (), ("bwd_conv2_wgrad",)),
    "gru_layer0": (lambda n: n.startswith("gru.") and "_l0" in n, (), ("bwd_gru_dw_l0",)),
    # frozen statistics AND frozen gamma / beta with trainable weights below: the frozen dz runs with no reduce / finalise before it
    "bn2_affine_and_stats": (lambda n: n in ("bn2.weight", "bn2.bias"), (2,), ()),
    "bn3_affine_and_stats": (lambda n: n in ("bn3.weight", "bn3.bias"), (1, 2, 3), ()),
}


@pytest.mark.parametrize("which", list(PRUNE_SETS))
@pytest.mark.parametrize("bsz", [256, 21])
def test_pruned_backward_is_bit_identical_and_skips_launches(sd, which, bsz):
    """requires_grad == False: no gradient, no launch that only feeds it, and every trainable gradient bit-identical to the full
    backward's in the same BatchNorm mode -- in the one-stream form (profiling on, where the launch counts are read) and in the
    two-stream form, three runs."""
    frozen, bn_eval, skipped = PRUNE_SETS[which]
    lib, h = _native.lib(), get_featurizer().handle
    x = cases.varied_features(bsz, 200, seed=700 + bsz).to(DEV)
    y = synth.synth_labels(bsz, 31, seed=701 + bsz).to(DEV)
    full = _model(sd, frozen_bn=bn_eval)
    _step(full, x, y)
    ref = {n: p.grad.clone() for n, p in full.named_parameters()}
    m = _model(sd, frozen_bn=bn_eval)
    _freeze_names(m, frozen)

    def check(tag):
        for n, p in m.named_parameters():
            if frozen(n):
                assert p.grad is None, (tag, n)
            else:
                assert torch.equal(p.grad, ref[n]), (tag, n, (p.grad - ref[n]).abs().max().item())

    for rep in range(3):                                    # two-stream form
        _step(m, x, y)
        check(("two", rep))
    nk = lib.sir_profile_kernel_count()
    names = [lib.sir_profile_kernel_name(i).decode() for i in range(nk)]
    ms, cnt = (C.c_double * nk)(), (C.c_int64 * nk)()
    _native.check(lib.sir_profile_enable(h, 1, -1), "sir_profile_enable")
    try:
        _step(m, x, y)
    finally:
        lib.sir_profile_collect(h, ms, cnt, nk)
        _native.check(lib.sir_profile_enable(h, 0, -1), "sir_profile_enable")
    check(("one", 0))
    counts = {names[i]: cnt[i] for i in range(nk) if names[i] in BWD_IDS}
    print(which, bsz, "backward launch counts:", counts)
    assert set(counts) == set(BWD_IDS)
    for k in BWD_IDS:
        assert (counts[k] == 0) == (k in skipped), (k, counts[k])


def test_three_adam_steps_over_trainable_subset_follow_reference(sd, golden):
    """conv / bn parameters and all statistics frozen, FusedAdam over the rest: the loss of each of three steps within 1e-4 of the
    reference's (the trajectory test's bound), sampled parameters within that test's per-step Adam bound x 3, frozen tensors
    and BatchNorm buffers bit-unchanged."""
    inp = cases.model_inputs()
    x, y = inp["x_train8"].to(DEV), inp["y_train8"].to(DEV)
    m = _model(sd)
    finetune.freeze(m, {"bn_stats", "cnn"})
    before = {k: v.clone() for k, v in m.state_dict().items()}
    opt = FusedAdam(finetune.trainable_parameters(m), lr=cases.LR, weight_decay=cases.WEIGHT_DECAY)
    losses = []
    for _ in range(3):
        m.train()                                           # the per-epoch model.train() must not undo the freeze
        opt.zero_grad(set_to_none=True)
        loss = train_ops.fused_cross_entropy(m(x), y)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    torch.cuda.synchronize()
    print("losses", losses, "golden", golden["head3/loss"].tolist())
    assert np.abs(np.asarray(losses) - golden["head3/loss"]).max() < 1e-4
    for name, p in m.named_parameters():
        if name.startswith(CNN):
            assert torch.equal(p, before[name]) and p.grad is None, name
            continue
        flat = p.detach().cpu().flatten()
        idx = cases.sample_indices(name, flat.numel())
        d = np.abs(flat[idx].numpy() - golden[f"head3/param_samp/{name}"])
        assert np.quantile(d, 0.9) <= 3 * 2e-6 and d.max() <= 3 * 2.1 * cases.LR, (name, d.max())
    for k, v in m.state_dict().items():
        if "running" in k or "tracked" in k:
            assert torch.equal(v, before[k]), k


@pytest.fixture(scope="module")
def nccl_group():
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29879")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        yield dist.group.WORLD
    finally:
        if dist.is_initialized():                         # (train() ends with shutdown_distributed())
            dist.destroy_process_group()


@pytest.mark.parametrize("overlap", [True, False])
def test_frozen_cnn_step_over_rccl_is_bit_identical(sd, nccl_group, monkeypatch, overlap):
    """One-rank nccl group, exchange forced: the frozen-CNN step equals the single-process one bit for bit and completes (no
    unbalanced collective); a rank without a batch joins the same collectives and ends with zero gradients on the trainable
    tensors only."""
    inp = cases.model_inputs()
    x, y = inp["x_train8"].to(DEV), inp["y_train8"].to(DEV)

    def run():
        m = _model(sd)
        finetune.freeze(m, {"bn_stats", "cnn"})
        _, loss = _step(m, x, y)
        return m, loss

    monkeypatch.setattr(train_ops, "FORCE_EXCHANGE", False)
    m0, loss0 = run()
    monkeypatch.setattr(train_ops, "FORCE_EXCHANGE", True)
    monkeypatch.setattr(train_ops, "OVERLAP_GRAD_EXCHANGE", overlap)
    for rep in range(3):
        m1, loss1 = run()
        assert torch.equal(loss0, loss1)
        for (n, p), (_, q) in zip(m0.named_parameters(), m1.named_parameters()):
            if n.startswith(CNN):
                assert p.grad is None and q.grad is None, n
            else:
                assert torch.equal(p.grad, q.grad), (n, rep)
    m2 = _model(sd)
    finetune.freeze(m2, {"bn_stats", "cnn"})
    train_ops.zero_contribution_step(m2)
    torch.cuda.synchronize()
    for n, p in m2.named_parameters():
        if n.startswith(CNN):
            assert p.grad is None, n
        else:
            assert p.grad is not None and not p.grad.any(), n


LABELS = ["activate_lights", "deactivate_lights", "increase_volume", "decrease_volume"]


def test_train_entry_point_with_init_checkpoint_and_freeze(tmp_path):
    """``train()`` on a toy corpus of ``test_pipeline_gpu.py``'s kind: a 31-class checkpoint into a 5-class run with
    ``freeze: [bn_stats, cnn]``.  It runs; the conv / BN tensors and BN buffers of the saved ``best_model.pt`` equal the
    checkpoint's bit for bit, ``fc`` has 5 rows, and the GRU moved."""
    import json
    import types
    import pandas as pd
    from sir_amd.scripts import train as tr
    from sir_amd.scripts.utils import wav_io
    wav = tmp_path / "wav"
    os.makedirs(wav)
    clips = synth.synth_clips(16, 48000, seed=4321)
    rng = np.random.Generator(np.random.PCG64(1))
    rows = []
    for i in range(16):
        path = str(wav / f"utt{i:03d}.wav")
        wav_io.write_wav_pcm16(path, clips[i, :int(rng.integers(16000, 48000))], 16000)
        rows.append({"path": path, "label": LABELS[i % 4]})
    csv = tmp_path / "train_data.csv"
    pd.DataFrame(rows).to_csv(csv, index=False)
    lm = tmp_path / "label_map.json"
    lm.write_text(json.dumps({l: i for i, l in enumerate(sorted(LABELS))}))
    sd31 = synth.synth_state_dict(31, seed=0)
    ckpt = tmp_path / "fsc31.pt"
    torch.save({"model_state_dict": sd31, "epoch": 7}, ckpt)
    cfg = {"batch_size": 8, "num_workers": 0, "num_labels": 5, "lr": 1e-3, "weight_decay": 1e-4, "epochs": 4, "early_stop_patience": 5,
           "augment_prob": 0.0, "use_feature_cache": False, "cache_dir": str(tmp_path / "nocache"), "save_path": str(tmp_path / "ckpt"),
           "fused_features": True, "seed": 1, "init_checkpoint": str(ckpt), "freeze": ["bn_stats", "cnn"]}
    args = types.SimpleNamespace(train_csv=str(csv), val_csv=str(csv), label_map=str(lm))
    best = tr.train(args, cfg)
    assert 0.0 < best <= 1.0                              # (best_model.pt is written on an improvement over 0, train.py:281)
    out = torch.load(os.path.join(cfg["save_path"], "best_model.pt"))
    assert list(out.keys()) == list(sd31.keys())
    assert out["fc.weight"].shape == (5, 512) and out["fc.bias"].shape == (5,)
    for k, v in sd31.items():
        if k.startswith(("conv", "bn")):
            assert torch.equal(out[k].cpu(), v), k        # parameters, running statistics and num_batches_tracked alike
    assert not torch.equal(out["gru.weight_ih_l0"].cpu(), sd31["gru.weight_ih_l0"])
    assert not torch.equal(out["attention.weight"].cpu(), sd31["attention.weight"])
    # `freeze` as a YAML scalar
    best2 = tr.train(args, dict(cfg, freeze="bn_stats", epochs=1, save_path=str(tmp_path / "ckpt2")))
    assert 0.0 <= best2 <= 1.0
