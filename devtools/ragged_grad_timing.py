"""Cost of the ragged differentiable step (``model(x, lengths=...)`` with frozen BatchNorm statistics) beside the dense all-frozen step
of the same build and shape, by ``sir_profile_*`` in its one-stream form (every kernel group between events of its own: the sums are
GPU time of the launches, not wall time of an overlapped step).

Batch 256, t_frames 200, frames drawn uniformly from [8, 200] (fixed seed), dropout 0.5, all 29 gradients and dx wanted.  The two routes
alternate step by step behind a warm-up; each figure is the mean over ``--steps`` steps.  Prints one JSON object; ``--out FILE`` also
writes it there.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from sir_amd import _native, finetune, ops, synth, train_ops   # noqa: E402
from sir_amd.featurizer import get_featurizer                  # noqa: E402
from sir_amd.models.models import CNNAudioGRU                  # noqa: E402


def profiled(fn, steps):
    """{profile name: ms per step} of `steps` calls of fn with every kernel group timed"""
    lib, h = _native.lib(), get_featurizer().handle
    nk = lib.sir_profile_kernel_count() + _native.PROFILE_EXTRA_IDS
    names = [lib.sir_profile_kernel_name(i).decode() for i in range(nk)]
    ms, cnt = (C.c_double * nk)(), (C.c_int64 * nk)()
    _native.check(lib.sir_profile_enable(h, 1, -1), "sir_profile_enable")
    try:
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
    finally:
        lib.sir_profile_collect(h, ms, cnt, nk)
        _native.check(lib.sir_profile_enable(h, 0, -1), "sir_profile_enable")
    return {names[i]: ms[i] / steps for i in range(nk) if cnt[i]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    _native.require_hip()
    dev = torch.device("cuda", 0)
    n, t = args.batch, args.frames
    model = CNNAudioGRU(31)
    model.load_state_dict(synth.synth_state_dict(31, seed=0))
    model = model.to(dev).train()
    finetune.freeze(model, {"bn_stats"})
    model.train()
    frames = np.random.default_rng(args.seed).integers(8, t + 1, size=n).tolist()
    lengths = torch.tensor(frames, dtype=torch.int32, device=dev)
    x = synth.synth_features(n, t, seed=3).to(dev)
    y = synth.synth_labels(n, 31, seed=4).to(dev)

    def step(lens):
        leaf = x.detach().requires_grad_(True)
        for p in model.parameters():
            p.grad = None
        logits = model(leaf, lengths=lens) if lens is not None else model(leaf)
        train_ops.fused_cross_entropy(logits, y).backward()

    for _ in range(3):
        step(None)
        step(lengths)
    torch.cuda.synchronize()
    dense, ragged = {}, {}
    for _ in range(args.steps):                               # alternating, one step per profile window
        for acc, lens in ((dense, None), (ragged, lengths)):
            for k, v in profiled(lambda: step(lens), 1).items():
                acc[k] = acc.get(k, 0.0) + v / args.steps
    ops.check_status()
    tot = lambda d: sum(v for k, v in d.items() if k.startswith(("train_", "bwd_")))
    out = {"device": torch.cuda.get_device_name(0), "batch": n, "t_frames": t, "steps": args.steps,
           "frames_mean": float(np.mean(frames)), "gru_steps_mean": float(np.mean([f // 8 for f in frames])),
           "statistic": "mean ms per step over the steps, sir_profile one-stream form, forward + backward kernel groups",
           "dense_frozen_ms": round(tot(dense), 4), "ragged_ms": round(tot(ragged), 4), "ratio_ragged_over_dense": round(tot(ragged) / tot(dense), 3),
           "dense_groups_ms": {k: round(v, 4) for k, v in dense.items()}, "ragged_groups_ms": {k: round(v, 4) for k, v in ragged.items()}}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
