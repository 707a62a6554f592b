"""Timing of the slot-head calls against their single-head relatives, on one GPU, in one process, on one build (compare
figures of one run only).

Batch 256, layout (6, 14, 4) -- Fluent Speech Commands' action / object / location -- against the single-head calls at
num_classes 24 on the same logits.  Every call goes straight to the C entry point with its outputs allocated beforehand, so a
figure is launch + kernel time, not tensor allocation:
  sir_ce_loss_slots          vs  sir_ce_loss_soft    (second labels, lam, label smoothing 0.1, dlogits written)
  sir_classify_slots (k = 3) vs  sir_classify (k = 3)
  sir_eval_accumulate_slots  vs  sir_eval_accumulate (15 bins)
Median of 7 regions of 20 calls between HIP events.  The yardstick is the single-head call: ``ratio`` is slot / single, to be
read against n_slots = 3.  Prints one JSON object; ``--out FILE`` also writes it there.
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

from sir_amd import _native, metrics, ops, slots                # noqa: E402
from sir_amd.featurizer import get_featurizer                   # noqa: E402

REGIONS = 7
BATCH, SIZES, K, BINS = 256, (6, 14, 4), 3, 15


def event_ms(fn, reps=20):
    fn()
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REGIONS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    return round(float(np.median(ms)), 5)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    _native.require_hip()
    dev = torch.device("cuda", 0)
    lib, h, st = _native.lib(), get_featurizer().handle, _native.current_stream_ptr()
    total, g_n = sum(SIZES), len(SIZES)
    gen = torch.Generator().manual_seed(11)
    logits = (torch.randn(BATCH, total, generator=gen) * 3).to(dev)
    ya = torch.stack([torch.randint(0, c, (BATCH,), generator=gen) for c in SIZES], dim=1).to(dev)
    yb = torch.stack([torch.randint(0, c, (BATCH,), generator=gen) for c in SIZES], dim=1).to(dev)
    y1, y1b = torch.randint(0, total, (BATCH,), generator=gen).to(dev), torch.randint(0, total, (BATCH,), generator=gen).to(dev)
    lam = torch.rand(BATCH, generator=gen).to(dev)
    sizes = (C.c_int32 * g_n)(*SIZES)
    loss, slot_loss, d = torch.empty(1, device=dev), torch.empty(g_n, device=dev), torch.empty_like(logits)
    idx_s = torch.empty((BATCH, g_n, K), dtype=torch.int32, device=dev)
    top_s, joint = torch.empty((BATCH, g_n, K), device=dev), torch.empty(BATCH, device=dev)
    idx_1, top_1 = torch.empty((BATCH, K), dtype=torch.int32, device=dev), torch.empty((BATCH, K), device=dev)
    state_s = torch.zeros(slots.state_words(SIZES, BINS), dtype=torch.int64, device=dev)
    state_1 = torch.zeros(metrics.state_words(total, BINS), dtype=torch.int64, device=dev)

    def check(rc):
        if rc != 0:
            raise _native.SirError(lib.sir_last_error().decode(errors="replace"))

    calls = {
        "sir_ce_loss_slots": lambda: check(lib.sir_ce_loss_slots(h, logits.data_ptr(), ya.data_ptr(), yb.data_ptr(), lam.data_ptr(), 0.1, sizes,
                                                                 None, g_n, BATCH, total, loss.data_ptr(), slot_loss.data_ptr(), d.data_ptr(), 1.0, st)),
        "sir_ce_loss_soft": lambda: check(lib.sir_ce_loss_soft(h, logits.data_ptr(), y1.data_ptr(), y1b.data_ptr(), lam.data_ptr(), 0.1, BATCH,
                                                               total, loss.data_ptr(), d.data_ptr(), 1.0, st)),
        "sir_classify_slots": lambda: check(lib.sir_classify_slots(h, logits.data_ptr(), BATCH, total, sizes, g_n, None, K, None, idx_s.data_ptr(),
                                                                   top_s.data_ptr(), joint.data_ptr(), st)),
        "sir_classify": lambda: check(lib.sir_classify(h, logits.data_ptr(), BATCH, total, None, K, None, idx_1.data_ptr(), top_1.data_ptr(), st)),
        "sir_eval_accumulate_slots": lambda: check(lib.sir_eval_accumulate_slots(h, logits.data_ptr(), ya.data_ptr(), BATCH, total, sizes, g_n, None,
                                                                                 BINS, state_s.data_ptr(), state_s.numel() * 8, st)),
        "sir_eval_accumulate": lambda: check(lib.sir_eval_accumulate(h, logits.data_ptr(), y1.data_ptr(), BATCH, total, None, BINS,
                                                                     state_1.data_ptr(), state_1.numel() * 8, st)),
    }
    ms = {name: event_ms(fn) for name, fn in calls.items()}
    pairs = [("sir_ce_loss_slots", "sir_ce_loss_soft"), ("sir_classify_slots", "sir_classify"), ("sir_eval_accumulate_slots", "sir_eval_accumulate")]
    res = {"device": torch.cuda.get_device_name(0), "batch": BATCH, "layout": list(SIZES), "single_head_classes": total,
           "statistic": f"median of {REGIONS} regions of 20 calls between HIP events, milliseconds per call", "kernel_ms": ms,
           "ratio_slot_over_single": {a: round(ms[a] / ms[b], 2) for a, b in pairs}, "n_slots": g_n}
    ops.check_status()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
