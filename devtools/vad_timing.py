"""Timing of the utterance segmenter on one GPU, in one process (compare figures of one run only).

64 ten-minute int16 recordings at 16 kHz resident in HBM (seeded: bursts of 1-3 s of noise separated by 1.5-6 s of near silence):
  segment   sir_vad_segment (chunk energy + state machine + table) at the listener's defaults
  gather    sir_vad_gather of the found segments, cut at the longest one (at most 200 frames' worth of samples)
  features  sir_features_fwd over the same number of samples, as [1024, 48000] batches, in the same session
  host      the same segmentation with tests/vad_ref.py (numpy) on the host, once, with a host clock
Each GPU figure is the median of 5 timed regions between HIP events, behind a warm-up.  "read GB/s" is the bytes of the recordings
(every sample once) over the segment time.  Prints one JSON object; ``--out FILE`` also writes it there.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import vad_ref                                                 # noqa: E402
from sir_amd import _native, ops                               # noqa: E402
from sir_amd.featurizer import HOP, get_featurizer             # noqa: E402
from sir_amd.segmenter import Segmenter                        # noqa: E402

REGIONS = 5
SR = 16000


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def median_ms(fn, reps):
    fn()
    fn()
    torch.cuda.synchronize()
    ms = [timed(fn, reps) for _ in range(REGIONS)]
    return float(np.median(ms)), [round(x, 4) for x in ms]


def make_recordings(n_rec, seconds, seed, dev):
    """int16 [n_rec, seconds * SR] on the GPU: per 1024-sample chunk an amplitude (0.1 inside a burst, 0.001 outside) times noise"""
    rng = np.random.default_rng(seed)
    n_chunks = seconds * SR // 1024
    amp = np.full((n_rec, n_chunks), 0.001, dtype=np.float32)
    for r in range(n_rec):
        t = rng.uniform(0.0, 3.0)
        while t < seconds:
            d = rng.uniform(1.0, 3.0)
            amp[r, int(t * SR / 1024):int((t + d) * SR / 1024) + 1] = 0.1
            t += d + rng.uniform(1.5, 6.0)
    g = torch.Generator(device=dev).manual_seed(seed)
    wave = torch.empty((n_rec, n_chunks * 1024), dtype=torch.int16, device=dev)
    a = torch.from_numpy(amp).to(dev)
    for r in range(n_rec):                                     # row by row: the float32 noise of one recording at a time
        x = torch.randn((n_chunks, 1024), generator=g, device=dev) * a[r, :, None]
        wave[r] = (x.clamp_(-1.0, 1.0) * 32767.0).round_().to(torch.int16).reshape(-1)
    return wave


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--recordings", type=int, default=64)
    ap.add_argument("--seconds", type=int, default=600)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    _native.require_hip()
    dev = torch.device("cuda", 0)
    wave = make_recordings(args.recordings, args.seconds, args.seed, dev)
    n_rec, length = wave.shape
    lengths = torch.full((n_rec,), length, dtype=torch.int32, device=dev)
    seg = Segmenter()
    table, seg_count, total = seg.segment(wave, lengths)       # sizes the table; later calls do not regrow
    n_seg = table.shape[0]
    longest = int((table[:, 2] - table[:, 1]).max().item())
    max_clip = min(longest, 200 * HOP - 1)
    seg_ms, seg_raw = median_ms(lambda: seg.segment(wave, lengths), 10)
    gat_ms, gat_raw = median_ms(lambda: seg.gather(wave, table, total, max_clip), 10)
    both_ms, both_raw = median_ms(lambda: seg.gather(wave, *seg.segment(wave, lengths)[::2], max_clip), 10)

    fz = get_featurizer()
    per = 1024 * 48000
    n_batches = max(1, wave.numel() // per)
    flat = wave.reshape(-1)
    batches = [flat[i * per:(i + 1) * per].view(1024, 48000) for i in range(n_batches)] if wave.numel() >= per else [flat[: flat.numel() // 48000 * 48000].view(-1, 48000)]
    covered = sum(b.numel() for b in batches)
    out = torch.empty((batches[0].shape[0], 64, 200), dtype=torch.float32, device=dev)

    def features():
        for b in batches:
            fz(b, t_pad=200, out=out)
    feat_ms, feat_raw = median_ms(features, 2)
    feat_same = feat_ms * wave.numel() / covered
    ops.check_status()

    host_s, same = None, None
    if not args.skip_host:
        w = wave.cpu().numpy()
        t0 = time.perf_counter()
        counts, ref = vad_ref.segment_batch(w, [length] * n_rec, seg.chunk_size, seg.threshold, seg.prior_chunks, seg.silence_chunks, True)
        host_s = time.perf_counter() - t0
        same = bool(np.array_equal(ref, table.cpu().numpy()) and np.array_equal(counts, seg_count.cpu().numpy()))

    bytes_read = wave.numel() * wave.element_size()
    res = {
        "device": torch.cuda.get_device_name(0), "recordings": n_rec, "seconds_each": args.seconds, "dtype": "int16",
        "samples": wave.numel(), "bytes_read": bytes_read, "segments": n_seg, "max_clip_len": max_clip,
        "regions": REGIONS, "statistic": "median ms per call over the regions (HIP events), one host read of `total` per segment call",
        "segment_ms": round(seg_ms, 4), "segment_read_GBps": round(bytes_read / seg_ms / 1e6, 1),
        "gather_ms": round(gat_ms, 4), "gather_written_bytes": n_seg * max_clip * 4,
        "segment_plus_gather_ms": round(both_ms, 4), "segment_plus_gather_read_GBps": round(bytes_read / both_ms / 1e6, 1),
        "features_ms_same_samples": round(feat_same, 3), "features_batches": f"{len(batches)} x {list(batches[0].shape)}",
        "host_vad_ref_s": None if host_s is None else round(host_s, 3), "host_table_equals_gpu": same,
        "regions_ms": {"segment": seg_raw, "gather": gat_raw, "segment_plus_gather": both_raw, "features": feat_raw},
    }
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
