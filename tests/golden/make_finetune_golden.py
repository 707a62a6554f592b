"""Generate ``finetune_golden.npz``: the REFERENCE's own ``CNNAudioGRU`` (CPU, fp32) driven with the torch fine-tuning idiom

    model.train(); bnK.eval() for the frozen blocks; requires_grad_(False) on the frozen layers

on the seeded inputs / weights of ``make_golden.py`` (``x_train8`` / ``y_train8``, ``synth_state_dict(31, seed=0)``, ``gru.dropout = 0``).
Run beside ``make_golden.py``, where the reference is available:

    python tests/golden/make_finetune_golden.py

Cases (outputs only; a few tens of KB):
* ``frozen/``  all three BatchNorm blocks in eval(): loss, logits, 64 sampled elements + norm of each of the 29 gradients, running
  statistics after the step (they must equal the checkpoint's).
* ``mixed/``   bn1 in eval(), bn2 / bn3 live: the same, with bn2 / bn3's updated running statistics.
* ``head3/``   conv / bn parameters frozen + all statistics frozen, three Adam steps over the trainable rest: the loss of every step
  and sampled parameters after the third.
``*/near_ties`` records how many 2x2 pooling windows of the reference had their two largest positive values within 1e-6 of each
other (where a device rounding could route the gradient to another pixel).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cases  # noqa: E402
from cases import LR, WEIGHT_DECAY  # noqa: E402

from sir_amd import synth  # noqa: E402

CASES = {"frozen": (1, 2, 3), "mixed": (1,)}
TRAJ_STEPS = 3


def _model(sd, frozen_bn):
    from models.models import CNNAudioGRU  # the reference itself
    model = CNNAudioGRU(31)
    model.load_state_dict(sd)
    model.train()
    model.gru.dropout = 0.0
    for i in frozen_bn:
        getattr(model, f"bn{i}").eval()
    return model


def _count_near_ties(model, x):
    ties = []

    def hook(mod, args):
        a = args[0].detach()
        b, c, h, w = a.shape
        win = a[:, :, : h // 2 * 2, : w // 2 * 2].reshape(b, c, h // 2, 2, w // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(b, c, h // 2, w // 2, 4)
        top = win.topk(2, dim=-1).values
        ties.append(int(((top[..., 0] > 0) & ((top[..., 0] - top[..., 1]).abs() <= 1e-6)).sum()))

    hd = model.pool.register_forward_pre_hook(hook)
    with torch.no_grad():
        model(x)
    hd.remove()
    return ties


def main():
    sys.path.insert(0, "/root/reference")
    nthr = torch.get_num_threads()
    torch.set_num_threads(1)                          # regenerates bit for bit whatever the host's core count
    try:
        sd = synth.synth_state_dict(31, seed=0)
        inp = cases.model_inputs()
        x, y = inp["x_train8"], inp["y_train8"]
        crit = torch.nn.CrossEntropyLoss()
        out = {}
        for case, frozen in CASES.items():
            model = _model(sd, frozen)
            ties = _count_near_ties(model, x)         # (no_grad forward in the same mode: live blocks update their statistics,
            model = _model(sd, frozen)                #  so the step itself runs on a fresh model)
            logits = model(x)
            loss = crit(logits, y)
            loss.backward()
            out[f"{case}/near_ties"] = np.asarray(ties, np.int64)
            out[f"{case}/loss"] = np.float32(loss.item())
            out[f"{case}/logits"] = logits.detach().numpy()
            for name, p in model.named_parameters():
                g = p.grad.detach().flatten()
                idx = cases.sample_indices(name, g.numel())
                out[f"{case}/grad_norm/{name}"] = np.float32(g.double().norm().item())
                out[f"{case}/grad_samp/{name}"] = g[idx].numpy()
            for i in (1, 2, 3):
                bn = getattr(model, f"bn{i}")
                out[f"{case}/bn{i}.running_mean"] = bn.running_mean.numpy()
                out[f"{case}/bn{i}.running_var"] = bn.running_var.numpy()
                out[f"{case}/bn{i}.num_batches_tracked"] = np.int64(bn.num_batches_tracked.item())
            print(case, "loss", loss.item(), "near ties per block", ties)

        model = _model(sd, (1, 2, 3))
        for n, p in model.named_parameters():
            if n.startswith(("conv", "bn")):
                p.requires_grad_(False)
        opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=LR, weight_decay=WEIGHT_DECAY)
        losses = []
        for _ in range(TRAJ_STEPS):
            opt.zero_grad(set_to_none=True)
            logits = model(x)
            loss = crit(logits, y)
            loss.backward()
            opt.step()
            losses.append(loss.item())
        out["head3/loss"] = np.asarray(losses, np.float32)
        for name, p in model.named_parameters():
            flat = p.detach().flatten()
            idx = cases.sample_indices(name, flat.numel())
            out[f"head3/param_samp/{name}"] = flat[idx].numpy()
        print("head3 losses", losses)
    finally:
        torch.set_num_threads(nthr)
    path = os.path.join(HERE, "finetune_golden.npz")
    np.savez_compressed(path, **out)
    print("finetune_golden.npz:", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
