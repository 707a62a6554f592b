"""Timing of the reverb / background-noise stage on one GPU, in one process (compare figures of one run only).

256 float32 clips of 48000 samples resident in HBM:
  reverb_mix   sir_wave_reverb_mix alone for RIRs of K = 1024, 4000 and 8192 taps (every row reverberated), without and with
               background noise, and the noise stage alone; median of 5 timed regions between HIP events, behind a warm-up
  features     sir_features_fwd over the same batch, in the same session
  epoch        train_epoch_waveforms over `--batches` batches of 256 (FeaturePrefetcher: the stage runs on the prefetch stream
               beside the training step), with the stage off and on (K = 8192 + noise on every row); the two legs are
               interleaved, `--rounds` times each, and the medians of their clips / s are reported with every round's figure
Prints one JSON object; ``--out FILE`` also writes it there.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from sir_amd import _native, ops, synth                        # noqa: E402
from sir_amd.featurizer import get_featurizer                  # noqa: E402
from sir_amd.sound_bank import SoundBank                       # noqa: E402

REGIONS = 5
B, L = 256, 48000


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def median_ms(fn, reps=10):
    fn()
    fn()
    torch.cuda.synchronize()
    ms = [timed(fn, reps) for _ in range(REGIONS)]
    return round(float(np.median(ms)), 4), [round(x, 4) for x in ms]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batches", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-epoch", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    _native.require_hip()
    dev = torch.device("cuda", 0)
    fz = get_featurizer()
    gen = np.random.default_rng(0)
    wave = synth.synth_clips(B, L, seed=1).to(dev)
    lengths = torch.full((B,), L, dtype=torch.int32, device=dev)
    noise = SoundBank([synth.coloured_noise(10 * 16000, gen, exponent=e) for e in (0.0, 1.0, 2.0, 1.0)], dev)
    idx = lambda n: torch.from_numpy(gen.integers(0, n, B).astype(np.int32)).to(dev)
    nkw = dict(noise=noise, noise_index=idx(len(noise)), noise_offset=idx(150000), snr_db=torch.full((B,), 10.0, device=dev))
    out = torch.empty((B, L), dtype=torch.float32, device=dev)
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "samples": L, "regions": REGIONS,
           "statistic": "median ms per call over the regions (HIP events, 10 calls per region)", "reverb_mix_ms": {}, "regions_ms": {}}
    banks = {}
    for k in (1024, 4000, 8192):
        rirs = [synth.synthetic_rir(1.0, rng=gen)[:k] for _ in range(16)]
        banks[k] = SoundBank(rirs, dev, kind="rir")
        assert banks[k].max_len == k
        rkw = dict(rir=banks[k], rir_index=idx(16))
        for name, kw in ((f"K{k}", rkw), (f"K{k}+noise", dict(rkw, **nkw))):
            res["reverb_mix_ms"][name], res["regions_ms"][name] = median_ms(lambda: fz.reverb_mix(wave, lengths, out=out, **kw))
    res["reverb_mix_ms"]["noise_only"], res["regions_ms"]["noise_only"] = median_ms(lambda: fz.reverb_mix(wave, lengths, out=out, **nkw))
    feats = torch.empty((B, 64, 200), dtype=torch.float32, device=dev)
    res["features_ms"], res["regions_ms"]["features"] = median_ms(lambda: fz(wave, lengths, t_pad=200, out=feats))
    ops.check_status()

    if not args.skip_epoch:
        from sir_amd.models.models import CNNAudioGRU
        from sir_amd.optim import FusedAdam
        from sir_amd.scripts import train as tr
        model = CNNAudioGRU(31)
        model.load_state_dict(synth.synth_state_dict(31, seed=0))
        model = model.to(dev).train()
        opt = FusedAdam(model.parameters(), lr=5e-5, weight_decay=1e-4)
        crit = torch.nn.CrossEntropyLoss()
        labels = synth.synth_labels(B).to(dev)
        host_lengths = [L] * B
        on_kw = dict(rir=banks[8192], rir_index=idx(16), **nkw)

        def leg(on):
            loader = [(wave, lengths, labels, host_lengths) for _ in range(args.batches)]
            aug = (lambda i, n, hl: on_kw) if on else None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.train_epoch_waveforms(model, loader, opt, crit, dev, t_pad=200, augment=aug)
            torch.cuda.synchronize()
            return args.batches * B / (time.perf_counter() - t0)
        leg(False)
        leg(True)                                               # warm-up of both legs
        rates = {"off": [], "on": []}
        for _ in range(args.rounds):                            # interleaved legs
            rates["off"].append(round(leg(False), 1))
            rates["on"].append(round(leg(True), 1))
        res["epoch_clips_per_s"] = {k: round(float(np.median(v)), 1) for k, v in rates.items()}
        res["epoch_rounds_clips_per_s"] = rates
        res["epoch_ms_per_step"] = {k: round(B / float(np.median(v)) * 1e3, 4) for k, v in rates.items()}
        res["epoch_batches"] = args.batches
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
