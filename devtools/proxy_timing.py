"""Timing of the cosine-proxy loss (sir_proxy_loss) against torch's own way to the same loss and gradients, and of the training
step with and without ``metric_loss``, on one GPU, on one build (compare figures of one run only).

Batch 256 embeddings against 31, 336 and 4096 proxies, scale 16, margin 0.1:
  sir_proxy_loss                 four launches: unit vectors, the row kernel (logits, loss, dz, demb), the proxy kernel (dproxies),
                                 the loss reduce -- loss and both gradients
  torch                          the yardstick on the same tensors: F.normalize, matmul, the margin, F.cross_entropy, backward
  step / step_metric_P           one training step at batch 256 x 200 frames (forward, loss, backward, FusedAdam): the classifier's
                                 cross-entropy alone, and with a ProxyHead of P proxies beside it
Every sir_proxy_loss call goes straight to the C entry point with its outputs allocated beforehand.  Routes are timed alternately,
two passes each; a pass is 7 regions of 20 calls between HIP events; the better pass's median stands, min / max over all regions.

``--mode step`` times the plain step alone and uses nothing that an older tree lacks; ``--root DIR`` imports the package from
another checkout (built there).  ``--parent-root DIR`` makes the default mode run ``--mode step`` in fresh child processes, this tree
and that one alternately (two each), and report both with their region-to-region spread: the plain step launches what it launched
before, so it must sit inside the parent's own spread.  Prints one JSON object; ``--out FILE`` also writes it there.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

REGIONS = 7
BATCH, FRAMES, CLASSES = 256, 200, 31
BANKS = (31, 336, 4096)
SCALE, MARGIN = 16.0, 0.1


def event_ms(fn, reps=20):
    import torch
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
    return ms


def summary(passes):
    """passes: lists of region times -> the better pass's median, min / max over all regions"""
    every = [v for p in passes for v in p]
    return {"median": round(min(float(np.median(p)) for p in passes), 5), "min": round(min(every), 5), "max": round(max(every), 5)}


def make_step(metric_proxies=None):
    """-> a callable running one training step at batch 256 x 200 frames"""
    import torch
    from sir_amd import synth, train_ops
    from sir_amd.models.models import CNNAudioGRU
    from sir_amd.optim import FusedAdam
    dev = torch.device("cuda", 0)
    model = CNNAudioGRU(CLASSES)
    model.load_state_dict(synth.synth_state_dict(CLASSES, seed=0))
    model = model.to(dev).train()
    x = synth.synth_features(BATCH, FRAMES, seed=7).to(dev)
    y = synth.synth_labels(BATCH, CLASSES, seed=8).to(dev)
    params = [p for p in model.parameters()]
    head = None
    if metric_proxies:
        from sir_amd.prototypes import ProxyHead
        head = ProxyHead(metric_proxies, scale=SCALE, margin=MARGIN, seed=0).to(dev)
        opt = FusedAdam([{"params": params}, {"params": [head.proxies]}], lr=1e-4)
    else:
        opt = FusedAdam(params, lr=1e-4)

    def step():
        opt.zero_grad(set_to_none=True)
        if head is None:
            loss = train_ops.fused_cross_entropy(model(x), y)
        else:
            logits, emb = model.forward_with_embedding(x)
            loss = train_ops.fused_cross_entropy(logits, y) + head(emb, y)
        loss.backward()
        opt.step()

    return step


def step_mode():
    from sir_amd import _native, ops
    _native.require_hip()
    passes = [event_ms(make_step()) for _ in range(2)]
    ops.check_status()
    return {"step": summary(passes), "regions": [[round(v, 5) for v in p] for p in passes]}


def child_step(root):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", "step", "--root", root], capture_output=True, text=True,
                         timeout=600)
    if out.returncode != 0:
        raise RuntimeError(f"--mode step in {root} failed:\n{out.stderr[-2000:]}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def all_mode(parent_root, own_root):
    import torch
    import torch.nn.functional as F
    from sir_amd import _native, ops
    from sir_amd.featurizer import get_featurizer
    _native.require_hip()
    dev = torch.device("cuda", 0)
    lib, h, st = _native.lib(), get_featurizer().handle, _native.current_stream_ptr()
    gen = torch.Generator().manual_seed(11)
    emb = (torch.randn(BATCH, 512, generator=gen) * 3).to(dev)
    labels = torch.randint(0, CLASSES, (BATCH,), generator=gen).to(dev)
    loss, demb = torch.empty((), device=dev), torch.empty_like(emb)
    ms, agree = {}, {}
    for n in BANKS:
        proxies = torch.randn(n, 512, generator=gen).to(dev)
        dprox = torch.empty_like(proxies)
        need = lib.sir_proxy_loss_workspace_bytes(BATCH, n)
        ws = torch.empty((need,), dtype=torch.uint8, device=dev)

        def fused(proxies=proxies, dprox=dprox, ws=ws, n=n, need=need):
            rc = lib.sir_proxy_loss(h, emb.data_ptr(), proxies.data_ptr(), labels.data_ptr(), BATCH, n, SCALE, MARGIN, loss.data_ptr(),
                                    demb.data_ptr(), dprox.data_ptr(), 1.0, ws.data_ptr(), need, st)
            if rc != 0:
                raise _native.SirError(lib.sir_last_error().decode(errors="replace"))

        et, pt = emb.clone().requires_grad_(True), proxies.clone().requires_grad_(True)

        def by_torch(et=et, pt=pt, n=n):
            et.grad = pt.grad = None
            z = SCALE * (F.normalize(et, dim=1) @ F.normalize(pt, dim=1).T - MARGIN * F.one_hot(labels, n))
            out = F.cross_entropy(z, labels)
            out.backward()
            return out

        runs = {"sir_proxy_loss": [], "torch_normalize_matmul_ce_backward": []}
        for _ in range(2):
            runs["sir_proxy_loss"].append(event_ms(fused))
            runs["torch_normalize_matmul_ce_backward"].append(event_ms(by_torch))
        for name, r in runs.items():
            ms[f"{name}_{n}"] = summary(r)
        fused()
        ref = by_torch()
        agree[str(n)] = {"loss_difference": abs(float(loss) - float(ref)),
                         "max_abs_demb_difference": float((demb - et.grad).abs().max()),
                         "max_abs_dproxies_difference": float((dprox - pt.grad).abs().max())}
    steps = {"step": make_step()}
    steps.update({f"step_metric_{n}": make_step(n) for n in BANKS})
    runs = {k: [] for k in steps}
    for _ in range(2):
        for k, fn in steps.items():
            runs[k].append(event_ms(fn))
    for k, r in runs.items():
        ms[k] = summary(r)
    res = {"device": torch.cuda.get_device_name(0), "batch": BATCH, "frames": FRAMES, "banks": list(BANKS), "scale": SCALE, "margin": MARGIN,
           "statistic": f"per route two passes, alternated; a pass is {REGIONS} regions of 20 calls between HIP events; median = the "
                        "better pass's median, min / max over all regions; milliseconds per call",
           "ms": ms, "agreement_with_torch": agree,
           "fused_over_torch": {str(n): round(ms[f"sir_proxy_loss_{n}"]["median"] / ms[f"torch_normalize_matmul_ce_backward_{n}"]["median"], 3)
                                for n in BANKS},
           "metric_step_over_step": {str(n): round(ms[f"step_metric_{n}"]["median"] / ms["step"]["median"], 4) for n in BANKS}}
    ops.check_status()
    if parent_root:
        torch.cuda.synchronize()
        own, parent = [], []
        for _ in range(2):                               # fresh processes, alternated: this tree, the parent's, ...
            own.append(child_step(own_root))
            parent.append(child_step(parent_root))
        res["plain_step_this_tree"] = summary([p for c in own for p in c["regions"]])
        res["plain_step_parent_tree"] = summary([p for c in parent for p in c["regions"]])
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mode", choices=("all", "step"), default="all")
    ap.add_argument("--root", type=str, default=None, help="the checkout to import sir_amd from (default: this file's)")
    ap.add_argument("--parent-root", type=str, default=None, help="a built checkout of the parent commit to time the plain step in")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    root = os.path.abspath(args.root) if args.root else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    res = step_mode() if args.mode == "step" else all_mode(args.parent_root, root)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
