"""Timing of joint decoding (sir_decode_slots) against the independent decoding it complements (sir_classify_slots), on one
GPU, in one process, on one build (compare figures of one run only).

Batch 256, layout (6, 14, 4) -- Fluent Speech Commands' action / object / location -- k = 3, the same logits for every call:
  sir_classify_slots                          the yardstick
  sir_decode_slots, table of 31 rows          the size of a closed intent set
  sir_decode_slots, table of 4096 rows        the largest table (rows drawn with repetition: the kernel does not care)
  sir_decode_slots, unconstrained             staged merging over the product space
each decode once with only the four required outputs and once with valid_mass and tuple_logp written too.  Every call goes
straight to the C entry point with its outputs allocated beforehand, so a figure is launch + kernel time, not tensor allocation.
Median of 7 regions of 20 calls between HIP events.  Prints one JSON object; ``--out FILE`` also writes it there.
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

from sir_amd import _native, ops, slots                         # noqa: E402
from sir_amd.featurizer import get_featurizer                   # noqa: E402

REGIONS = 7
BATCH, SIZES, K = 256, (6, 14, 4), 3
TABLES = (31, 4096)


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
    sizes = (C.c_int32 * g_n)(*SIZES)
    rng = np.random.default_rng(5)
    tables = {}
    for n in TABLES:
        rows = np.stack([rng.integers(0, c, n) for c in SIZES], axis=1)
        tables[n] = torch.from_numpy(slots.pack_tuples(rows, g_n)).to(dev)
    idx_s = torch.empty((BATCH, g_n, K), dtype=torch.int32, device=dev)
    top_s, joint = torch.empty((BATCH, g_n, K), device=dev), torch.empty(BATCH, device=dev)
    index = torch.empty((BATCH, K), dtype=torch.int32, device=dev)
    labels = torch.empty((BATCH, K, g_n), dtype=torch.int32, device=dev)
    logp, prob, mass = torch.empty((BATCH, K), device=dev), torch.empty((BATCH, K), device=dev), torch.empty(BATCH, device=dev)
    scores = torch.empty((BATCH, max(TABLES)), device=dev)

    def check(rc):
        if rc != 0:
            raise _native.SirError(lib.sir_last_error().decode(errors="replace"))

    def decode(table, n, extras):
        return lambda: check(lib.sir_decode_slots(h, logits.data_ptr(), BATCH, total, sizes, g_n, None,
                                                  table.data_ptr() if table is not None else None, n, K, index.data_ptr(),
                                                  labels.data_ptr(), logp.data_ptr(), prob.data_ptr(),
                                                  mass.data_ptr() if extras else None,
                                                  scores.data_ptr() if extras and table is not None else None, st))

    calls = {"sir_classify_slots": lambda: check(lib.sir_classify_slots(h, logits.data_ptr(), BATCH, total, sizes, g_n, None, K, None,
                                                                        idx_s.data_ptr(), top_s.data_ptr(), joint.data_ptr(), st))}
    for n in TABLES:
        calls[f"sir_decode_slots_table_{n}"] = decode(tables[n], n, False)
        calls[f"sir_decode_slots_table_{n}_mass_scores"] = decode(tables[n], n, True)
    calls["sir_decode_slots_unconstrained"] = decode(None, 0, False)
    calls["sir_decode_slots_unconstrained_mass"] = decode(None, 0, True)
    ms = {name: event_ms(fn) for name, fn in calls.items()}
    res = {"device": torch.cuda.get_device_name(0), "batch": BATCH, "layout": list(SIZES), "k": K,
           "statistic": f"median of {REGIONS} regions of 20 calls between HIP events, milliseconds per call", "kernel_ms": ms,
           "ratio_over_classify_slots": {a: round(v / ms["sir_classify_slots"], 2) for a, v in ms.items() if a != "sir_classify_slots"}}
    ops.check_status()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
