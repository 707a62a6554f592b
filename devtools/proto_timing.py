"""Timing of the prototype head (sir_proto_score) against torch's own way to the same answer, and of sir_model_embed against
sir_model_infer, on one GPU, in one process, on one build (compare figures of one run only).

Batch 256 embeddings against 64, 336 and 4096 unit prototypes (class = row), k = 3:
  sir_proto_score                             one launch: normalise, similarities, top-3 classes, softmax, nearest prototype
  sir_proto_score + sims                      the same with the [256][P] similarity matrix written out too
  torch                                       the yardstick: normalize(emb) @ protos.T, then topk(3) -- on the same tensors
The torch route does less (no probabilities, no nearest row).  Every sir call goes straight to the C entry point with its
outputs allocated beforehand, so a figure is launch + kernel time, not tensor allocation.  The two routes are timed alternately.
sir_model_embed / sir_model_infer: batch 256 x 200 frames, prepared weights reused, with and without the classifier.
Median of 7 regions of 20 calls (model: 5 calls) between HIP events.  Prints one JSON object; ``--out FILE`` also writes it there.
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

from sir_amd import _native, ops, synth                         # noqa: E402
from sir_amd.featurizer import get_featurizer                   # noqa: E402
from sir_amd.models.models import CNNAudioGRU                   # noqa: E402

REGIONS = 7
BATCH, K = 256, 3
BANKS = (64, 336, 4096)


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
    return round(float(np.median(ms)), 5), round(float(min(ms)), 5), round(float(max(ms)), 5)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    _native.require_hip()
    dev = torch.device("cuda", 0)
    lib, h, st = _native.lib(), get_featurizer().handle, _native.current_stream_ptr()
    gen = torch.Generator().manual_seed(11)
    emb = (torch.randn(BATCH, 512, generator=gen) * 3).to(dev)
    cls = torch.empty((BATCH, K), dtype=torch.int32, device=dev)
    sim, prob = torch.empty((BATCH, K), device=dev), torch.empty((BATCH, K), device=dev)
    nearest = torch.empty((BATCH,), dtype=torch.int32, device=dev)

    def check(rc):
        if rc != 0:
            raise _native.SirError(lib.sir_last_error().decode(errors="replace"))

    ms, agree = {}, {}
    for n in BANKS:
        protos = torch.nn.functional.normalize(torch.randn(n, 512, generator=gen), dim=1).to(dev)
        sims = torch.empty((BATCH, n), device=dev)

        def fused(want_sims, protos=protos, sims=sims, n=n):
            return lambda: check(lib.sir_proto_score(h, emb.data_ptr(), BATCH, protos.data_ptr(), None, None, n, n, None, K,
                                                     sims.data_ptr() if want_sims else None, cls.data_ptr(), sim.data_ptr(),
                                                     prob.data_ptr(), nearest.data_ptr(), st))

        def by_torch(protos=protos):
            return torch.topk(torch.nn.functional.normalize(emb, dim=1) @ protos.T, K, dim=1)

        # alternate the routes: two passes each, the better median of a route stands (the spread is reported beside it)
        runs = {"sir_proto_score": [], "sir_proto_score_sims": [], "torch_normalize_matmul_topk": []}
        for _ in range(2):
            runs["sir_proto_score"].append(event_ms(fused(False)))
            runs["torch_normalize_matmul_topk"].append(event_ms(by_torch))
            runs["sir_proto_score_sims"].append(event_ms(fused(True)))
        for name, r in runs.items():
            ms[f"{name}_{n}"] = {"median": min(x[0] for x in r), "min": min(x[1] for x in r), "max": max(x[2] for x in r)}
        fused(True)()
        tv, ti = by_torch()
        agree[str(n)] = {"top1_equal": bool(torch.equal(ti[:, 0].to(torch.int32), cls[:, 0])),
                         "max_abs_sim_difference": float((tv - sim).abs().max())}

    model = CNNAudioGRU(31)
    model.load_state_dict(synth.synth_state_dict(31, seed=0))
    model = model.to(dev).eval()
    x = synth.synth_features(BATCH, 200, seed=7).to(dev)
    model_runs = {"sir_model_infer": [], "sir_model_embed_with_logits": [], "sir_model_embed": []}
    for _ in range(2):
        model_runs["sir_model_infer"].append(event_ms(lambda: ops.model_infer(model, x, model._ws, want_argmax=True), reps=5))
        model_runs["sir_model_embed_with_logits"].append(event_ms(lambda: ops.model_embed(model, x, model._ws, want_logits=True), reps=5))
        model_runs["sir_model_embed"].append(event_ms(lambda: ops.model_embed(model, x, model._ws), reps=5))
    for name, r in model_runs.items():
        ms[name] = {"median": min(v[0] for v in r), "min": min(v[1] for v in r), "max": max(v[2] for v in r)}
    res = {"device": torch.cuda.get_device_name(0), "batch": BATCH, "k": K, "banks": list(BANKS),
           "statistic": f"per route two passes, alternated; a pass is {REGIONS} regions of 20 calls (model: 5) between HIP events; "
                        "median = the better pass's median, min / max over all regions; milliseconds per call",
           "ms": ms, "agreement_with_torch": agree,
           "fused_over_torch": {str(n): round(ms[f"sir_proto_score_{n}"]["median"] / ms[f"torch_normalize_matmul_topk_{n}"]["median"], 3)
                                for n in BANKS},
           "embed_over_infer": round(ms["sir_model_embed_with_logits"]["median"] / ms["sir_model_infer"]["median"], 4)}
    ops.check_status()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
