"""Runs only the feature kernel (batch 256, 3 s clips) -- for rocprofv3 passes and quick timings.
usage: python3 devtools/feat_only.py [iters] [i16|f32] [aug] [--backward]
--backward: also times sir_features_bwd beside the forward in the same process, both with HIP events around regions of `iters`
launches (median of 7 regions after a warm-up region), and prints the ratio."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from sir_amd.featurizer import get_featurizer  # noqa: E402

backward = "--backward" in sys.argv
sys.argv = [a for a in sys.argv if a != "--backward"]
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
i16 = len(sys.argv) > 2 and sys.argv[2] == "i16"
aug = len(sys.argv) > 3 and sys.argv[3] == "aug"
dev = torch.device("cuda", 0)
g = torch.Generator(device=dev).manual_seed(1)
pool = [(0.1 * torch.randn(256, 48000, generator=g, device=dev)).clamp_(-1, 1) for _ in range(8)]
if i16:
    pool = [(p * 32767).round().to(torch.int16) for p in pool]
lengths = torch.full((256,), 48000, dtype=torch.int32, device=dev)
out = torch.empty(256, 64, 200, device=dev)
fz = get_featurizer()
kw = {}
if aug:
    kw = dict(shift=torch.randint(-4800, 4800, (256,), dtype=torch.int32, device=dev),
              noise_sigma=torch.full((256,), 0.005, device=dev), noise_seed=5)
for i in range(3):
    fz(pool[i % 8], lengths, t_pad=200, out=out, **kw)
torch.cuda.synchronize()
t0 = time.perf_counter()
for i in range(iters):
    fz(pool[i % 8], lengths, t_pad=200, out=out, **kw)
torch.cuda.synchronize()
print(f"feature stage: {(time.perf_counter() - t0) / iters * 1e6:.1f} us per batch of 256 ({'i16' if i16 else 'f32'}{', aug' if aug else ''})")

if backward:
    import statistics
    db = torch.empty(256, 64, 200, device=dev)
    dout = torch.randn(256, 64, 200, generator=g, device=dev)
    dwave = torch.empty(256, 48000, device=dev)

    def region(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(iters):
            fn(pool[i % 8])
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / iters

    def fwd(w):
        fz(w, lengths, t_pad=200, out=out, db_out=db, **kw)

    def bwd(w):
        fz.features_bwd(w, lengths, db, dout, t_pad=200, out=dwave, **kw)

    fwd(pool[0])                          # db of pool[0]: the backward's statistics stay sane for every wave of the pool
    times = {"forward": [], "backward": []}
    for rep in range(8):                  # region 0 is the warm-up; the two kernels alternate region by region
        for name, fn in (("forward", fwd), ("backward", bwd)):
            t = region(fn)
            if rep:
                times[name].append(t)
    f, b = statistics.median(times["forward"]), statistics.median(times["backward"])
    print(f"events, median of 7 regions of {iters}: forward {f:.1f} us, backward {b:.1f} us, ratio {b / f:.2f} "
          f"(min {min(times['forward']):.1f} / {min(times['backward']):.1f})")
