"""Timing of the live-stream segmenter on one GPU, in one process (compare figures of one run only).

S = 1024 streams, int16, 1024 new samples per stream and push (64 ms of audio at 16 kHz), the listener's defaults.  The audio is
seeded: bursts of 1-3 s of noise separated by 1.5-6 s of near silence, a different phase per stream, so utterances end all the time.
  push      sir_stream_push (append + chunk energy + state machine), per push, over a run of `--pushes` consecutive pushes
  gather    sir_stream_gather of the rows each push emitted, cut at 200 frames' worth of samples, per push over the same run.
            Launched over the whole table (`sir_stream_max_rows` rows, all but a few of them beyond `total`) because the host does
            not read `total` here; `StreamSegmenter.push` reads it and launches over the emitted rows only
  nothing   the same run with pushes of 0 samples (nothing to append, no chunk to judge): the fixed cost of a push -- three
            launches and the state machine's walk over S streams.  Per-kernel times come from a kernel trace of this tool
            (rocprofv3 --kernel-trace --stats, in a run of its own): profiles/stream/README.md
  batch     sir_vad_segment + sir_vad_gather over the same total samples held as [S, pushes * 1024] recordings
Each figure is the median of 5 timed regions between HIP events, behind a warm-up run; a region is one whole run of pushes, its time
divided by their number.  `total` is not read by the host inside a region (the table is sized for the worst case), so the figures
are device time per push, not the latency of a host loop.  Prints one JSON object; ``--out FILE`` also writes it there.

``--input-rate HZ`` and / or ``--encoding pcm|ulaw|alaw`` time the stream input stage instead (sir_stream_input_push in front of
sir_stream_push): one push of a float32 segmenter that is handed 1024 samples at 16 kHz per stream, against one push of a segmenter
with the front stage that is handed the same 64 ms at the callers' rate and codec (512 bytes at 8 kHz mu-law), same process, raw
library calls, no host read inside a region, median of 7 regions.
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

from sir_amd import _native, ops                               # noqa: E402
from sir_amd.featurizer import HOP                             # noqa: E402
from sir_amd.segmenter import Segmenter                        # noqa: E402
from sir_amd.streaming import StreamSegmenter                  # noqa: E402

REGIONS = 5
SR = 16000


def region_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def median_ms(fn, per):
    fn()
    torch.cuda.synchronize()
    ms = [region_ms(fn) / per for _ in range(REGIONS)]
    return float(np.median(ms)), [round(x, 5) for x in ms]


def make_audio(n_streams, n_chunks, seed, dev):
    """int16 [n_streams, n_chunks * 1024]: per chunk an amplitude (0.1 inside a burst, 0.001 outside) times noise"""
    rng = np.random.default_rng(seed)
    seconds = n_chunks * 1024 / SR
    amp = np.full((n_streams, n_chunks), 0.001, dtype=np.float32)
    for r in range(n_streams):
        t = rng.uniform(-3.0, 3.0)
        while t < seconds:
            d = rng.uniform(1.0, 3.0)
            amp[r, max(0, int(t * SR / 1024)):max(0, int((t + d) * SR / 1024) + 1)] = 0.1
            t += d + rng.uniform(1.5, 6.0)
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn((n_streams, n_chunks, 1024), generator=g, device=dev) * torch.from_numpy(amp).to(dev)[:, :, None]
    return (x.clamp_(-1.0, 1.0) * 32767.0).round_().to(torch.int16).reshape(n_streams, -1)


def front_stage(args, dev):
    """push with and without the stream input stage at the same number of 16 kHz samples"""
    from sir_amd import g711
    regions, S, n_push = 7, args.streams, min(args.pushes, 64)
    rate = args.input_rate or SR
    enc = args.encoding or "pcm"
    per_in = 1024 * rate // SR
    if per_in < 1:
        raise SystemExit(f"--input-rate {rate}: a push of 64 ms holds no sample")
    n_chunks = max(n_push, -(-n_push * per_in // 1024))             # enough audio for n_push pushes at either rate
    pcm = make_audio(S, n_chunks, args.seed, dev)                   # int16 [S, n_chunks * 1024]
    plain = StreamSegmenter(S, 1024, dtype=torch.float32, device=dev)
    plain.reset()
    wave16 = pcm[:, :n_push * 1024].float() / 32768.0
    src = pcm[:, :n_push * per_in].contiguous()                      # the same kind of signal, read at the callers' rate
    assert src.shape[1] == n_push * per_in and wave16.shape[1] == n_push * 1024
    if enc != "pcm":
        src = torch.from_numpy(g711.encode(src.cpu().numpy(), enc)).to(dev)
    front = StreamSegmenter(S, per_in, device=dev, input_rate=rate, encoding=enc)
    front.reset()
    lib, st = _native.lib(), _native.current_stream_ptr()
    full16 = torch.full((S,), 1024, dtype=torch.int32, device=dev)
    full_in = torch.full((S,), per_in, dtype=torch.int32, device=dev)
    esz = src.element_size()

    def seg_push(ss, ptr, stride, width, lengths):
        rc = lib.sir_stream_push(ss._handle, ss._state.data_ptr(), ss._state.numel(), C.byref(ss._cfg), ptr, stride, width, lengths.data_ptr(),
                                 None, None, ss._table.data_ptr(), ss.max_rows, ss._total.data_ptr(), st)
        _native.check(rc, "sir_stream_push")

    def run_plain():
        plain.reset()
        for k in range(n_push):
            seg_push(plain, wave16.data_ptr() + 4 * 1024 * k, wave16.stride(0), 1024, full16)

    si = front.input
    conv = front._converted
    conv_len = torch.zeros((S,), dtype=torch.int32, device=dev)

    def front_only(k):
        rc = lib.sir_stream_input_push(si._handle, si._state.data_ptr(), si._state.numel(), C.byref(si._cfg), src.data_ptr() + esz * per_in * k,
                                       src.stride(0), per_in, full_in.data_ptr(), None, conv.data_ptr(), conv.stride(0), conv_len.data_ptr(), st)
        _native.check(rc, "sir_stream_input_push")

    def run_front(segment=True):
        front.reset()
        for k in range(n_push):
            front_only(k)
            if segment:
                seg_push(front, conv.data_ptr(), conv.stride(0), conv.shape[1], conv_len)

    def med(fn):
        fn()
        torch.cuda.synchronize()
        ms = [region_ms(fn) / n_push for _ in range(regions)]
        return round(float(np.median(ms)), 5), [round(x, 5) for x in ms]
    plain_ms, plain_raw = med(run_plain)
    front_ms, front_raw = med(run_front)
    stage_ms, stage_raw = med(lambda: run_front(False))
    ops.check_status()
    return {"device": torch.cuda.get_device_name(0), "streams": S, "pushes_per_region": n_push, "regions": regions,
            "input_rate": rate, "encoding": enc, "input_dtype": str(si.dtype), "samples_in_per_push": per_in, "samples_16k_per_push": 1024,
            "front_max_out": si.max_out, "front_state_bytes": si._state.numel(),
            "statistic": "median over the regions of (HIP-event time of a run of pushes / pushes), ms per push; no host read inside a region",
            "push_without_front_ms": plain_ms, "push_with_front_ms": front_ms, "front_stage_alone_ms": stage_ms,
            "regions_ms": {"without_front": plain_raw, "with_front": front_raw, "front_stage_alone": stage_raw}}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--input-rate", type=int, default=None, help="time the stream input stage: the callers' sample rate (Hz)")
    ap.add_argument("--encoding", type=str, default=None, choices=["pcm", "ulaw", "alaw"], help="time the stream input stage: the callers' codec")
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--pushes", type=int, default=256, help="consecutive pushes of one timed region (256 = 16.4 s of audio per stream)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    _native.require_hip()
    dev = torch.device("cuda", 0)
    if args.input_rate is not None or args.encoding is not None:
        res = front_stage(args, dev)
        print(json.dumps(res))
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
        return
    S, n_push = args.streams, args.pushes
    wave = make_audio(S, n_push, args.seed, dev)
    ss = StreamSegmenter(S, 1024, dtype=torch.int16, device=dev)
    ss.reset()
    lib, h, cfg = _native.lib(), ss._handle, ss._cfg
    state, table, total = ss._state, ss._table, ss._total
    full = torch.full((S,), 1024, dtype=torch.int32, device=dev)
    none = torch.zeros((S,), dtype=torch.int32, device=dev)
    max_clip = 200 * HOP - 1
    clips = torch.empty((ss.max_rows, -(-max_clip // 4) * 4), dtype=torch.float32, device=dev)      # rows 16-byte aligned: vector stores
    clip_len = torch.empty((ss.max_rows,), dtype=torch.int32, device=dev)
    rows_seen = torch.zeros((1,), dtype=torch.int64, device=dev)
    st = _native.current_stream_ptr()

    def push(k, lengths):
        rc = lib.sir_stream_push(h, state.data_ptr(), state.numel(), C.byref(cfg), wave.data_ptr() + 2 * 1024 * k, wave.stride(0), 1024,
                                 lengths.data_ptr(), None, None, table.data_ptr(), ss.max_rows, total.data_ptr(), st)
        _native.check(rc, "sir_stream_push")

    def gather():
        rc = lib.sir_stream_gather(h, state.data_ptr(), state.numel(), C.byref(cfg), table.data_ptr(), total.data_ptr(), ss.max_rows,
                                   clips.data_ptr(), clips.stride(0), max_clip, clip_len.data_ptr(), st)
        _native.check(rc, "sir_stream_gather")

    def run(with_gather, lengths=full, count=False):
        ss.reset()
        for k in range(n_push):
            push(k, lengths)
            if count:
                rows_seen.add_(total[0])
            if with_gather:
                gather()

    run(False, count=True)
    n_rows = int(rows_seen.item())
    reset_ms, reset_raw = median_ms(lambda: ss.reset(), 1)
    push_ms, push_raw = median_ms(lambda: run(False), n_push)
    both_ms, both_raw = median_ms(lambda: run(True), n_push)
    idle_ms, idle_raw = median_ms(lambda: run(False, none), n_push)

    seg = Segmenter()
    lengths = torch.full((S,), wave.shape[1], dtype=torch.int32, device=dev)
    btable, _, btotal = seg.segment(wave, lengths)                 # sizes the table; later calls do not regrow
    longest = int((btable[:, 2] - btable[:, 1]).max().item()) if btable.shape[0] else 1
    bclip = min(longest, max_clip)
    bseg_ms, bseg_raw = median_ms(lambda: seg.segment(wave, lengths), 1)
    bboth_ms, bboth_raw = median_ms(lambda: seg.gather(wave, *seg.segment(wave, lengths)[::2], bclip), 1)
    ops.check_status()

    audio_ms = 1024 * 1000.0 / SR
    res = {
        "device": torch.cuda.get_device_name(0), "streams": S, "samples_per_push": 1024, "dtype": "int16", "pushes_per_region": n_push,
        "audio_ms_per_push": audio_ms, "ring_chunks": ss.ring_chunks, "max_utt_chunks": ss.max_utt_chunks, "state_bytes": state.numel(),
        "bytes_appended_per_push": S * 1024 * 2, "rows_emitted_per_region": n_rows, "gather_grid_rows": ss.max_rows,
        "max_clip_len": max_clip, "regions": REGIONS,
        "statistic": "median over the regions of (HIP-event time of a run of pushes / pushes), ms per push; no host read inside a region",
        "push_ms": round(push_ms, 5), "push_plus_gather_ms": round(both_ms, 5), "gather_ms_by_difference": round(both_ms - push_ms, 5),
        "push_of_nothing_ms": round(idle_ms, 5), "reset_ms": round(reset_ms, 5),
        "realtime_factor_push_plus_gather": round(audio_ms / both_ms, 1),
        "batch_segment_ms_same_samples": round(bseg_ms, 4), "batch_segment_plus_gather_ms_same_samples": round(bboth_ms, 4),
        "batch_segments": int(btable.shape[0]), "batch_max_clip_len": bclip,
        "stream_push_plus_gather_ms_same_samples": round(both_ms * n_push, 4),
        "regions_ms": {"push": push_raw, "push_plus_gather": both_raw, "push_of_nothing": idle_raw, "reset": reset_raw,
                       "batch_segment": bseg_raw, "batch_segment_plus_gather": bboth_raw},
    }
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
