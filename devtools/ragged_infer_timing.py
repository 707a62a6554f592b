"""Timing of the un-padded ("ragged") batch inference on one GPU, in one process (compare figures of one run only).

A. 256 clips, lengths drawn uniformly from 30..200 frames (seeded):
     (a) one at a time through the single-clip un-padded path (``model(x[b:b+1, :, :frames[b]])``: a whole launch sequence at B = 1,
         a new (B, T) shape -- and so a rebuild of the prepared weights -- for every new length),
     (b) as ONE ragged batch (``model(x, lengths=frames)``).
B. frames = [94] * 256 at t_frames = 200: the ragged call against ``sir_model_infer`` on the same zero-padded features (pad skip).

Each figure is the median of 5 timed regions between HIP events, every region behind a warm-up of all the shapes it uses; the two
routes of a comparison alternate region by region.  Prints one JSON object; ``--out FILE`` also writes it there.
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

from sir_amd import _native, ops, synth                      # noqa: E402
from sir_amd.models.models import CNNAudioGRU                # noqa: E402

REGIONS = 5


def timed(fn, reps):
    """milliseconds per call of `fn` over one region of `reps` calls"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(routes, reps):
    """{name: median ms per call} over REGIONS regions per route, the routes alternating"""
    for fn in routes.values():                                # warm-up: every shape once, then once more
        fn()
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in routes}
    for _ in range(REGIONS):
        for k, fn in routes.items():
            ms[k].append(timed(fn, reps[k]))
    return {k: float(np.median(v)) for k, v in ms.items()}, {k: [round(x, 4) for x in v] for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    _native.require_hip()
    dev = torch.device("cuda", 0)
    n = args.clips
    model = CNNAudioGRU(31)
    model.load_state_dict(synth.synth_state_dict(31, seed=0))
    model = model.to(dev).eval()
    rng = np.random.default_rng(args.seed)
    frames = rng.integers(30, 201, size=n).tolist()
    t_max = max(frames)
    x = synth.synth_features(n, t_max, seed=3).to(dev)
    for b, f in enumerate(frames):
        x[b, :, f:] = 0.0
    clips = [x[b:b + 1, :, :f].contiguous() for b, f in enumerate(frames)]
    lengths = torch.tensor(frames, dtype=torch.int32, device=dev)

    with torch.no_grad():
        def one_at_a_time():
            for c in clips:
                model(c)

        def ragged():
            model(x, lengths=lengths)

        med_a, raw_a = alternate({"one_at_a_time": one_at_a_time, "ragged_batch": ragged}, {"one_at_a_time": 1, "ragged_batch": 20})
        # the two routes agree (the ragged rows are the single-clip logits up to another tiling of the same sums)
        single = torch.cat([model(c) for c in clips])
        diff = (single - model(x, lengths=lengths)).abs().max().item()

        x94 = synth.synth_features(n, 200, seed=4).to(dev)
        x94[:, :, 94:] = 0.0
        l94 = torch.full((n,), 94, dtype=torch.int32, device=dev)
        ws_p, ws_r = ops.Workspace(), ops.Workspace()
        med_b, raw_b = alternate({"padded_pad_skip": lambda: ops.model_infer(model, x94, ws_p),
                                  "ragged_94": lambda: ops.model_infer(model, x94, ws_r, lengths=l94)},
                                 {"padded_pad_skip": 20, "ragged_94": 20})
    ops.check_status()
    out = {
        "device": torch.cuda.get_device_name(0), "clips": n, "frames_min": min(frames), "frames_max": t_max,
        "regions": REGIONS, "statistic": "median ms per call over the regions (HIP events)",
        "A_one_at_a_time_ms": round(med_a["one_at_a_time"], 3), "A_ragged_batch_ms": round(med_a["ragged_batch"], 3),
        "A_speedup": round(med_a["one_at_a_time"] / med_a["ragged_batch"], 1), "A_max_abs_logit_difference": diff,
        "B_padded_pad_skip_ms": round(med_b["padded_pad_skip"], 4), "B_ragged_94_ms": round(med_b["ragged_94"], 4),
        "B_ratio_ragged_over_padded": round(med_b["ragged_94"] / med_b["padded_pad_skip"], 3),
        "regions_ms": {**raw_a, **raw_b},
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
