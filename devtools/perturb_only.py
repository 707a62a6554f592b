"""Times sir_wave_perturb (HipFeaturizer.perturb) alone, batch 256 x 3 s, device events after warm-up -- and the feature
stage with and without it in front.  For rocprofv3 --kernel-trace --stats passes run it in a process of its own.
usage: python3 devtools/perturb_only.py [iters] [both|pitch|tempo] [i16|f32]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from sir_amd.featurizer import get_featurizer  # noqa: E402

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 50
mode = sys.argv[2] if len(sys.argv) > 2 else "both"
i16 = len(sys.argv) > 3 and sys.argv[3] == "i16"
B, L = 256, 48000
dev = torch.device("cuda", 0)
g = torch.Generator(device=dev).manual_seed(1)
pool = [(0.1 * torch.randn(B, L, generator=g, device=dev)).clamp_(-1, 1) for _ in range(4)]
if i16:
    pool = [(p * 32767).round().to(torch.int16) for p in pool]
lengths = torch.full((B,), L, dtype=torch.int32, device=dev)
shift = torch.randint(-4800, 4800, (B,), dtype=torch.int32, device=dev, generator=g)
cents = (torch.rand(B, device=dev, generator=g) * 400 - 200).clamp_(-200, 200)       # every row drawn, none 0
cents = torch.where(cents == 0, torch.full_like(cents, 50.0), cents)
tempo = 0.85 + 0.3 * torch.rand(B, device=dev, generator=g)
tempo = torch.where(tempo == 1, torch.full_like(tempo, 1.05), tempo)
kw = dict(shift=shift, pitch_cents=cents if mode in ("both", "pitch") else None, tempo=tempo if mode in ("both", "tempo") else None)
fz = get_featurizer()
feats = torch.empty(B, 64, 200, device=dev)


def timed(fn):
    for i in range(5):
        fn(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def perturb(i):
    return fz.perturb(pool[i % 4], lengths, **kw)


def perturb_features(i):
    w, n = perturb(i)
    fz(w, n, t_pad=200, out=feats, noise_sigma=torch.full((B,), 0.005, device=dev), noise_seed=i)


def features(i):
    fz(pool[i % 4], lengths, t_pad=200, out=feats, shift=shift, noise_sigma=torch.full((B,), 0.005, device=dev), noise_seed=i)


tag = f"{mode}, {'i16' if i16 else 'f32'}"
print(f"perturb: {timed(perturb):.1f} us per batch of {B} x {L} ({tag})")
print(f"perturb + features: {timed(perturb_features):.1f} us; features alone (shift + noise fused): {timed(features):.1f} us")
