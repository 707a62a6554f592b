"""Host side of fine-tuning (no GPU): ``finetune.load_pretrained`` / ``freeze`` on CPU tensors, the ``model.train()`` interaction,
the new C ABI entries in header, binding and library, and the golden file's own invariants."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import cases
import finetune_ref
from sir_amd import _native, finetune, synth
from sir_amd.models.models import CNNAudioGRU

NEW_SYMBOLS = ("sir_model_train_fwd_cfg", "sir_model_train_bwd_cfg")


def test_header_binding_and_library_export_the_cfg_entries():
    header = open(os.path.join(cases.ROOT, "include", "sir_hip.h")).read()
    assert "typedef struct sir_train_config" in header and re.search(r"int\s+bn_frozen\[3\];", header)
    assert re.search(r"#define\s+SIR_ABI_VERSION\s+1\b", header)          # purely additive
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _native.SIGNATURES, name
    assert _native.SIGNATURES["sir_model_train_fwd_cfg"][1][10]._type_ is _native.TrainConfig
    assert _native.SIGNATURES["sir_model_train_bwd_cfg"][1][8]._type_ is _native.TrainConfig
    assert len(_native.SIGNATURES["sir_model_train_fwd_cfg"][1]) == len(_native.SIGNATURES["sir_model_train_fwd"][1]) + 1
    assert len(_native.SIGNATURES["sir_model_train_bwd_cfg"][1]) == len(_native.SIGNATURES["sir_model_train_bwd_part"][1]) + 1
    if not os.path.exists(_native.LIB_PATH):
        pytest.fail("libsir_hip.so is not built")
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NEW_SYMBOLS:
        assert name in exported, name


def test_load_pretrained_keeps_body_and_resets_a_mismatching_head():
    sd31 = synth.synth_state_dict(31, seed=0)
    torch.manual_seed(1)
    m = CNNAudioGRU(5)
    fc_before = m.fc.weight.detach().clone()
    rep = finetune.load_pretrained(m, {"model_state_dict": {"module." + k: v for k, v in sd31.items()}})
    assert sorted(rep["reset"]) == ["fc.bias", "fc.weight"] and sorted(rep["shape_mismatch"]) == ["fc.bias", "fc.weight"]
    assert not rep["missing"] and not rep["unexpected"]
    assert set(rep["kept"]) == set(sd31) - {"fc.weight", "fc.bias"}
    own = m.state_dict()
    for k in rep["kept"]:
        assert torch.equal(own[k], sd31[k]), k
    assert m.fc.weight.shape == (5, 512) and not torch.equal(m.fc.weight, fc_before)
    bound = 1.0 / np.sqrt(512)                                            # torch's default nn.Linear init
    assert m.fc.weight.abs().max() <= bound and m.fc.bias.abs().max() <= bound and m.fc.weight.std() > 0.3 * bound


def test_load_pretrained_same_label_set_raw_dict_path_and_options(tmp_path):
    sd31 = synth.synth_state_dict(31, seed=0)
    m = CNNAudioGRU(31)
    rep = finetune.load_pretrained(m, sd31)
    assert rep["reset"] == [] and set(rep["kept"]) == set(sd31)
    assert torch.equal(m.fc.weight, sd31["fc.weight"])
    path = tmp_path / "ckpt.pt"
    torch.save({"model_state_dict": sd31, "epoch": 3}, path)
    m2 = CNNAudioGRU(31)
    rep2 = finetune.load_pretrained(m2, str(path), reset_head=True)
    assert sorted(rep2["reset"]) == ["fc.bias", "fc.weight"] and not torch.equal(m2.fc.weight, sd31["fc.weight"])
    assert torch.equal(m2.conv2.weight, sd31["conv2.weight"])
    m3 = CNNAudioGRU(7)
    w0 = m3.fc.weight.detach().clone()
    rep3 = finetune.load_pretrained(m3, sd31, reset_head=False)
    assert rep3["reset"] == [] and torch.equal(m3.fc.weight, w0)
    partial = {k: v for k, v in sd31.items() if not k.startswith("attention.")}
    partial["extra.key"] = torch.zeros(1)
    rep4 = finetune.load_pretrained(CNNAudioGRU(31), partial)
    assert sorted(rep4["missing"]) == ["attention.bias", "attention.weight"] and rep4["unexpected"] == ["extra.key"]
    bad = dict(sd31)
    bad["conv1.weight"] = torch.zeros(16, 1, 3, 3)
    with pytest.raises(ValueError, match="conv1.weight"):
        finetune.load_pretrained(CNNAudioGRU(31), bad)
    with pytest.raises(TypeError):
        finetune.load_pretrained(CNNAudioGRU(31), 3)


def test_freeze_sets_flags_and_survives_model_train():
    m = CNNAudioGRU(5)
    with pytest.raises(ValueError, match="unknown"):
        finetune.freeze(m, {"fc"})
    trainable = finetune.freeze(m, ["bn_stats", "cnn"])
    assert not any(n.startswith(("conv", "bn")) for n in trainable) and "fc.weight" in trainable and len(trainable) == 20
    assert m.training and m.gru.training and not (m.bn1.training or m.bn2.training or m.bn3.training)
    m.eval()
    m.train()                                                             # the top of every epoch
    assert m.training and m.gru.training and not (m.bn1.training or m.bn2.training or m.bn3.training)
    assert [p.requires_grad for n, p in m.named_parameters() if n.startswith(("conv", "bn"))] == [False] * 9
    assert len(finetune.trainable_parameters(m)) == 20
    finetune.freeze(m, "gru")
    m.train()
    assert not m.gru.training and not any(p.requires_grad for p in m.gru.parameters())
    finetune.freeze(m, {"attention"})
    assert [n for n, p in m.named_parameters() if p.requires_grad] == ["fc.weight", "fc.bias"]
    plain = CNNAudioGRU(5)                                                # no freeze: nn.Module.train exactly
    plain.bn2.eval()
    plain.train()
    assert plain.bn2.training


def test_step_config_reads_submodule_flags():
    from sir_amd import train_ops
    m = CNNAudioGRU(5).train()
    cfg, p = train_ops.step_config(m)
    assert list(cfg.bn_frozen) == [0, 0, 0] and p == 0.5
    m.bn1.eval(); m.bn3.eval(); m.gru.eval()
    cfg, p = train_ops.step_config(m)
    assert list(cfg.bn_frozen) == [1, 0, 1] and p == 0.0


def test_golden_file_invariants():
    """What must hold in the reference's own numbers whatever the device does: frozen statistics did not move, the frozen step and
    the first step of the three-step run are the same computation, and the file is small."""
    path = os.path.join(cases.GOLDEN_DIR, "finetune_golden.npz")
    assert os.path.getsize(path) < 200 * 1024
    g = np.load(path)
    sd = synth.synth_state_dict(31, seed=0)
    for i in (1, 2, 3):
        assert np.array_equal(g[f"frozen/bn{i}.running_mean"], sd[f"bn{i}.running_mean"].numpy())
        assert np.array_equal(g[f"frozen/bn{i}.running_var"], sd[f"bn{i}.running_var"].numpy())
    assert np.array_equal(g["mixed/bn1.running_var"], sd["bn1.running_var"].numpy())
    assert not np.array_equal(g["mixed/bn2.running_var"], sd["bn2.running_var"].numpy())
    assert g["head3/loss"][0] == g["frozen/loss"] and g["head3/loss"][2] < g["head3/loss"][0]
    assert g["frozen/loss"] != g["mixed/loss"]
    for case in ("frozen", "mixed"):
        assert g[f"{case}/near_ties"].shape == (3,)
        assert len([k for k in g.files if k.startswith(f"{case}/grad_samp/")]) == 29


@pytest.mark.parametrize("case,frozen", [("frozen", (True, True, True)), ("mixed", (True, False, False))])
def test_finetune_ref_is_pinned_to_the_reference_golden(case, frozen):
    """``tests/finetune_ref.py`` against the reference's own module (CPU fp32 both): loss, logits, every gradient's 64 samples and norm,
    the running statistics after the step.  Bounds: those of ``test_oracle_golden.py`` for its training step (loss 1e-5, logits 2e-5,
    statistics rtol 1e-5) and the project's gradient bound 2e-3 of the tensor's rms -- 2e-2 for conv / bn, whose golden inputs have
    pooling windows within 1e-6 of a tie (``*/near_ties``) that two fp32 forwards may route differently."""
    g = np.load(os.path.join(cases.GOLDEN_DIR, "finetune_golden.npz"))
    sd = synth.synth_state_dict(31, seed=0)
    inp = cases.model_inputs()
    loss, grads, stats, logits = finetune_ref.loss_and_grads(sd, inp["x_train8"], inp["y_train8"], bn_frozen=frozen)
    assert abs(loss.item() - float(g[f"{case}/loss"])) < 1e-5
    np.testing.assert_allclose(logits.numpy(), g[f"{case}/logits"], rtol=0, atol=2e-5)
    assert len(grads) == 29
    for name, gr in grads.items():
        flat = gr.flatten()
        idx = cases.sample_indices(name, flat.numel())
        norm = float(g[f"{case}/grad_norm/{name}"])
        rms = norm / np.sqrt(flat.numel())
        tol = 2e-2 if name.startswith(("conv", "bn")) else 2e-3
        err = np.abs(flat[idx].numpy() - g[f"{case}/grad_samp/{name}"]).max()
        print(case, name, f"{err / (rms + 1e-30):.1e}")
        assert err <= tol * rms + 1e-7, name
        assert abs(flat.double().norm().item() - norm) <= 0.5 * tol * norm + 1e-7, name
    for i, fz in zip((1, 2, 3), frozen):
        for s_ in ("running_mean", "running_var"):
            if fz:
                assert np.array_equal(stats[f"bn{i}.{s_}"].numpy(), g[f"{case}/bn{i}.{s_}"])
            else:
                np.testing.assert_allclose(stats[f"bn{i}.{s_}"].numpy(), g[f"{case}/bn{i}.{s_}"], rtol=1e-5, atol=1e-6)


def test_finetune_ref_trainable_subset_and_frozen_backward_form():
    """A subset of ``trainable`` returns exactly those gradients, equal to the full call's; and the frozen block's backward is the
    affine form: d loss / d z = dy * gamma * invstd_running, checked on a tiny tensor against the closed form."""
    sd = synth.synth_state_dict(31, seed=0)
    x = cases.varied_features(2, 32, seed=11)
    y = torch.tensor([3, 7])
    _, full, _, _ = finetune_ref.loss_and_grads(sd, x, y, bn_frozen=(True, True, True))
    _, sub, _, _ = finetune_ref.loss_and_grads(sd, x, y, bn_frozen=(True, True, True), trainable={"fc.weight", "gru.bias_hh_l0", "bn3.bias"})
    assert sorted(sub) == ["bn3.bias", "fc.weight", "gru.bias_hh_l0"]
    for k, v in sub.items():
        assert torch.equal(v, full[k]), k
    z = torch.randn(2, 64, 4, 6, dtype=torch.float64, requires_grad=True)
    sd64 = {k: v.double() for k, v in sd.items()}
    out = finetune_ref.batchnorm(z, sd64, 2, True, {})
    dy = torch.randn_like(out)
    (dz,) = torch.autograd.grad(out, z, dy)
    inv = torch.rsqrt(sd64["bn2.running_var"] + 1e-5)
    assert torch.allclose(dz, dy * (sd64["bn2.weight"] * inv)[None, :, None, None], rtol=1e-12, atol=0)


def test_ranks_that_froze_different_sets_are_told_so(monkeypatch):
    """``train_ops._check_same_freeze``: the (digest, -digest) MAX-reduce agrees with the local digest only when every rank froze
    the same set; a peer with another set makes this rank raise, an equal peer does not, and an agreed set is checked once."""
    import torch.distributed as dist
    from sir_amd import train_ops
    calls = []

    def fake_all_reduce(peer_bits):
        def f(t, op=None):
            assert op == dist.ReduceOp.MAX
            calls.append(t.clone())
            t.copy_(torch.maximum(t, torch.tensor([peer_bits, -peer_bits], dtype=t.dtype)))
        return f

    cfg = _native.TrainConfig()
    cfg.bn_frozen[0] = 1
    need = (True,) * 9 + (False,) * 20
    mine = sum(1 << i for i in range(9)) + (1 << 29)
    monkeypatch.setattr(train_ops, "_freeze_checked", set())
    for peer in (mine - 1, mine + 4, 0):                         # a smaller, a larger and an empty digest on the other rank
        monkeypatch.setattr(dist, "all_reduce", fake_all_reduce(peer))
        with pytest.raises(_native.SirError, match="different"):
            train_ops._check_same_freeze(need, cfg, device="cpu")
    monkeypatch.setattr(dist, "all_reduce", fake_all_reduce(mine))
    train_ops._check_same_freeze(need, cfg, device="cpu")
    n = len(calls)
    train_ops._check_same_freeze(need, cfg, device="cpu")        # agreed: not reduced again
    assert len(calls) == n and calls[-1].tolist() == [mine, -mine]
