"""Runs only the feature kernel (batch 256, 3 s clips) -- for rocprofv3 passes and quick timings.
usage: python3 devtools/feat_only.py [iters] [i16|f32] [aug] [--backward] [--n-fft N[,N..] --hop H[,H..] --win W[,W..]]
--n-fft / --hop / --win: time the feature stage at other front-ends (comma-separated lists time several in the SAME run, e.g.
  --n-fft 512,1024,1024 --hop 160,256,512 --win 400,1024,1024: the last one is the specialised kernel, the yardstick); HIP events
  around regions of `iters` launches, median of 7 regions after a warm-up region, the configurations alternating region by
  region; prints microseconds per batch and nanoseconds per frame.  t_pad is the clips' frame count rounded up to 4.
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


def _take(flag):
    """value list of `flag` (removed from sys.argv), or None"""
    if flag not in sys.argv:
        return None
    i = sys.argv.index(flag)
    vals = [int(v) for v in sys.argv[i + 1].split(",")]
    del sys.argv[i:i + 2]
    return vals


n_ffts, hops, wins = _take("--n-fft"), _take("--hop"), _take("--win")
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

if n_ffts or hops or wins:
    import statistics
    n = max(len(v) for v in (n_ffts, hops, wins) if v)
    n_ffts = n_ffts or [1024] * n
    hops = hops or [f // 2 for f in n_ffts]
    wins = wins or list(n_ffts)
    runs = []
    for n_fft, hop, win in zip(n_ffts, hops, wins):
        t_pad = (1 + 48000 // hop + 3) // 4 * 4
        runs.append(((n_fft, hop, win), get_featurizer(16000, 64, n_fft, hop, win), t_pad,
                     torch.empty(256, 64, t_pad, device=dev), []))
    for rep in range(8):                  # region 0 is the warm-up
        for cfg, f, t_pad, o, ts in runs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(iters):
                f(pool[i % 8], lengths, t_pad=t_pad, out=o, **kw)
            e1.record()
            e1.synchronize()
            if rep:
                ts.append(e0.elapsed_time(e1) * 1e3 / iters)
    for cfg, f, t_pad, o, ts in runs:
        us, frames = statistics.median(ts), 256 * (1 + 48000 // cfg[1])
        print(f"n_fft {cfg[0]} hop {cfg[1]} win {cfg[2]}: {us:.1f} us per batch of 256 (min {min(ts):.1f}), {frames} frames, "
              f"{us * 1e3 / frames:.1f} ns per frame")

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
