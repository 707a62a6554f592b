"""Timing of adversarial training on one GPU, in one process (compare figures of one run only).

Batch 256 x 64 mels x 200 frames resident in HBM, the last 40 frames zero padding:
  adv_step     sir_adv_step alone: gradient step out of place, gradient step in place, random start, and the gradient step with
               keep_zero_columns off; median of 5 timed regions between HIP events (10 calls each), behind a warm-up; the
               effective bandwidth counts three reads and one write of the batch (one read, one write for the random start)
  step         one training step (zero_grad, forward, loss, backward, FusedAdam) with the adversary off and with
               Adversary(steps=1) and Adversary(steps=3) in front of it, each a region of `--steps` steps between HIP events;
               the three legs are interleaved, `--rounds` times each, and the medians are reported with every round's figure
               and the ratios against the plain step of the same run
Prints one JSON object; ``--out FILE`` also writes it there.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from sir_amd import _native, ops, synth, train_ops             # noqa: E402

REGIONS = 5
B, T, T_LIVE = 256, 200, 160


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def median_ms(fn, reps=10):
    fn()
    fn()
    torch.cuda.synchronize()
    ms = [timed(fn, reps) for _ in range(REGIONS)]
    return round(float(np.median(ms)), 4), [round(x, 4) for x in ms]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--eps", type=float, default=0.05)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    _native.require_hip()
    dev = torch.device("cuda", 0)
    x0 = synth.synth_features(B, T, seed=7)
    x0[:, :, T_LIVE:] = 0.0
    x0 = x0.to(dev)
    g = torch.randn(B, 64, T, device=dev)
    x = x0 + 0.01 * torch.randn(B, 64, T, device=dev)
    out = torch.empty_like(x0)
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "frames": T, "regions": REGIONS, "eps": args.eps,
           "statistic": "median ms per call over the regions (HIP events)", "adv_step_ms": {}, "adv_step_gb_per_s": {}, "regions_ms": {}}
    nbytes = x0.numel() * 4
    legs = {"grad": (lambda: train_ops.adv_step(x0, x, g, args.eps, 0.01, out=out), 4),
            "grad_in_place": (lambda: train_ops.adv_step(x0, x, g, args.eps, 0.01, out=x), 4),
            "grad_no_column_rule": (lambda: train_ops.adv_step(x0, x, g, args.eps, 0.01, keep_zero_columns=False, out=out), 4),
            "random_start": (lambda: train_ops.adv_step(x0, None, None, args.eps, 0.0, seed=12345, out=out), 2)}
    for name, (fn, passes) in legs.items():
        ms, regions = median_ms(fn)
        res["adv_step_ms"][name], res["regions_ms"][name] = ms, regions
        res["adv_step_gb_per_s"][name] = round(passes * nbytes / (ms * 1e-3) / 1e9, 1)
    ops.check_status()

    from sir_amd.models.models import CNNAudioGRU
    from sir_amd.optim import FusedAdam
    model = CNNAudioGRU(31)
    model.load_state_dict(synth.synth_state_dict(31, seed=0))
    model = model.to(dev).train()
    opt = FusedAdam(model.parameters(), lr=5e-5, weight_decay=1e-4)
    labels = synth.synth_labels(B).to(dev)
    adversaries = {"off": None, "steps1": train_ops.Adversary(args.eps, steps=1, random_start=True, seed=1),
                   "steps3": train_ops.Adversary(args.eps, steps=3, random_start=True, seed=1)}

    def step(adv):
        opt.zero_grad(set_to_none=True)
        mel = x0 if adv is None else adv(model, x0, lambda o: train_ops.fused_cross_entropy(o, labels))
        train_ops.fused_cross_entropy(model(mel), labels).backward()
        opt.step()

    for adv in adversaries.values():                            # warm-up of every leg
        for _ in range(3):
            step(adv)
    torch.cuda.synchronize()
    rounds = {k: [] for k in adversaries}
    for _ in range(args.rounds):                                # interleaved legs
        for name, adv in adversaries.items():
            rounds[name].append(round(timed(lambda: step(adv), args.steps), 4))
    ops.check_status()
    med = {k: round(float(np.median(v)), 4) for k, v in rounds.items()}
    res["train_step_ms"] = med
    res["train_step_rounds_ms"] = rounds
    res["ratio_to_plain_step"] = {k: round(med[k] / med["off"], 3) for k in ("steps1", "steps3")}
    res["train_steps_per_region"] = args.steps
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
