#!/usr/bin/env python3
"""Benchmark of the hot path: batched audio -> intent inference (and the training step) on MI355X.

    python bench.py --gpus N --steps K --warmup W

One "step" = one pass of the hot path over one batch of 256 synthetic 16 kHz / 3 s clips that
are already resident in HBM: fused HIP feature extraction (framed rFFT -> mel -> log -> z-norm ->
pad to 200 frames) followed by the HIP CNN/BiGRU/attention forward and argmax -- BASELINE.json
configs[1].  Utterances are independent, so N > 1 shards them (one process per GPU, 256 per GPU
per step, weak scaling) with no collective on the data path; torch.distributed (RCCL) is used only
for the barrier and the max-over-ranks of the elapsed time.  The training legs (`train`, `train_aug`
in the same JSON line: configs[2] / [3] / [4]) end every step in the RCCL all-reduce of the 13 MB gradient.

Launching: with --gpus N > 1 and no WORLD_SIZE in the environment this process is only a LAUNCHER: it
starts `python -m torch.distributed.run --nproc-per-node N bench.py ...` as a child BEFORE touching the
GPU (it never does), relays rank 0's JSON line and exits with the child's code.  Started by an external
launcher (WORLD_SIZE set) it is one rank; WORLD_SIZE != --gpus is an error, not a silent downgrade.

Every timed figure is the MEDIAN of `--repeats` (5) timed regions of exactly K steps, each bracketed by
barrier + synchronize on both sides and max-reduced over ranks; min / max are reported.

A plain run does only what the headline figure needs: set-up, W warm-up steps, the untimed per-kernel pass that picks
the kernel bracketed with HIP events in the timed regions, the timed regions, --dump-outputs, and ONE JSON line on rank 0
(value, ms_per_step, timed_regions, kernels_avg_ms, features_stage, gru_recurrence).  --full adds every other leg to
the same line:
  roofline       -- dominant kernel, achieved vs peak, timed live with HIP events on its stream (single-stream leg)
  single_stream  -- the same regions strictly serial
  sustained      -- >= --sustain-seconds of pipelined steps with package power / sclk
  train, train_aug -- the training-step legs (with rccl_world1, host_fed, dropin_epoch at N = 1)
  cpu_baseline   -- the CPU restatement of the reference path (oracle/, "port") timed on the host
                    cores of this box on a bounded sample (rank 0, N = 1 only), with the argmax parity flag

--dump-outputs DIR writes what the last timed inference step returned (features, logits, predicted indices) as .npy
files.  Clips and weights are seeded, so the same arguments give the same inputs on every run and two builds of the
project can be compared output for output.
"""
import argparse
import ctypes as C
import json
import os
import socket
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

BATCH = 256
CLIP_LEN = 48000
T_PAD = 200
NUM_CLASSES = 31
N_POOL = 8                       # distinct batches staged in HBM (8 x 49 MB > the 256 MB MALL)
PEAK_F32_MFMA_TFLOPS = 157.3     # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense
PEAK_BF16_MFMA_TFLOPS = 2500.0   # MI355X_MICROARCH.md: bf16 MFMA, dense (no sparsity)
# Round 4: every contraction of the path computes its fp32 products as THREE fp16 MFMA products ("f16x3": two-way fp16 split of both
# operands, csrc/f16_split.h / f16x3_kernels.h; rounds 1-3: six bf16 products, "bf16x6"): the matrix pipe executes 3x the
# algorithmic FLOPs, so the peak for ALGORITHMIC fp32 FLOP/s is 2500/3 = 833.3 TFLOP/s.  (With bf16x6 it was 2500/6 = 416.7: a
# fraction quoted against THAT peak in earlier rounds is twice the fraction of the same rate against this one.)
PEAK_F16X3_TFLOPS = 2500.0 / 3.0
# (rounds 1-3) six bf16 MFMA products per fp32 product: the matrix pipe executes 6x the algorithmic FLOPs, so the peak for
# ALGORITHMIC fp32 FLOP/s on that path is 2500/6 TFLOP/s
PEAK_BF16X6_TFLOPS = PEAK_BF16_MFMA_TFLOPS / 6.0
PEAK_HBM_GBS = 8000.0            # MI355X_MICROARCH.md: HBM3E spec peak
DUMP_LIMIT_BYTES = 64 * 10 ** 6  # --dump-outputs: every file of one run together, all ranks

# algorithmic work per utterance at T = 200 frames
_CONV2 = 2 * 64 * 288 * 32 * 100
_CONV3 = 2 * 128 * 576 * 16 * 50
_IH0 = 2 * 25 * 1024 * 1536
_IH1 = 2 * 25 * 512 * 1536
_REC = 2 * 25 * 2 * 768 * 256
FLOPS_PER_UTT = {
    "conv1_bn_relu_pool": 2 * 32 * 9 * 64 * 200,
    "conv2_mfma_bn_relu_pool": _CONV2, "conv3_mfma_bn_relu_pool": _CONV3,
    "gemm_ih_l0": _IH0, "gemm_ih_l1": _IH1, "gru_recurrence_l0": _REC, "gru_recurrence_l1": _REC,
    # training step: forward twins, data gradients (same contraction sizes) and weight gradients
    "train_conv1_fwd": 2 * 32 * 9 * 64 * 200, "train_conv2_fwd": _CONV2, "train_conv3_fwd": _CONV3,
    "train_gemm_ih_l0": _IH0, "train_gemm_ih_l1": _IH1, "train_gru_l0": _REC, "train_gru_l1": _REC,
    "bwd_gru_l1": _REC, "bwd_gru_l0": _REC,
    "bwd_gru_dw_l1": 2 * 25 * 1536 * (512 + 256), "bwd_gru_dw_l0": 2 * 25 * 1536 * (1024 + 256),
    "bwd_gru_dx_l1": _IH1, "bwd_gru_dx_l0": _IH0,
    "bwd_conv3_wgrad": _CONV3, "bwd_conv3_dgrad": _CONV3, "bwd_conv2_wgrad": _CONV2, "bwd_conv2_dgrad": _CONV2,
}
BF16X6_KERNELS = {k for k in FLOPS_PER_UTT if "conv1" not in k}      # the matrix-core kernels (all on f16x3 since round 4; the name is historic)
F16X3_KERNELS = BF16X6_KERNELS
# csrc/conv_wino2_bf16x6_kernel.h (producer / consumer Winograd kernel; SIR_WINO2 selects the stages, default all three)
WINOGRAD_KERNELS = {"conv2_mfma_bn_relu_pool", "conv3_mfma_bn_relu_pool", "train_conv2_fwd", "train_conv3_fwd", "bwd_conv3_dgrad",
                    "bwd_conv2_wgrad", "bwd_conv3_wgrad"}
# kernel symbol behind each profile id of the inference leg (several ids may share one symbol: the roofline block reports the
# largest single launch AND, as `by_symbol`, the symbol with the largest total time)
KERNEL_SYMBOL = {
    "feat_frames": "feat_utt_kernel<float,false>", "conv1_bn_relu_pool": "conv1_mfma_bn_relu_pool_kernel",
    "conv2_mfma_bn_relu_pool": "conv3x3_wino2_bf16x6_kernel<32,64,0,F16>", "conv3_mfma_bn_relu_pool": "conv3x3_wino2_bf16x6_kernel<64,128,1,F16>",
    "gemm_ih_l0": "gemm_nt_f16x3_kernel", "gemm_ih_l1": "gemm_nt_f16x3_kernel",
    "gru_recurrence_l0": "gru_quad_kernel<false, false>", "gru_recurrence_l1": "gru_quad_kernel<false, false>",
    "attention_pool_fc_argmax": "attention_pool_kernel",
}
FWD_FLOPS_PER_UTT = 400646144
TRAIN_FLOPS_PER_UTT = 3 * FWD_FLOPS_PER_UTT                  # fwd + dgrad + wgrad convention: 1 201 938 432
FEATURE_BYTES_PER_UTT = CLIP_LEN * 4 + 64 * T_PAD * 4       # 243 200 B (fp32 waveform in, features out)
# GRU recurrence, algorithmic HBM bytes per launch at B = 256 (gate pre-activations in, y out, + the bf16x3 planes of y
# that layer 0 writes for the next projection): VERDICT r1 item 6
GRU_ALGO_BYTES = {"gru_recurrence_l0": BATCH * 25 * (1536 * 4 + 512 * 4 + 512 * 6), "gru_recurrence_l1": BATCH * 25 * (1536 * 4 + 512 * 4)}


def log(msg):
    print(f"[bench] {msg}", file=sys.stderr, flush=True)


# ---- launcher (parent process; never touches the GPU) ---------------------------------------------------------------
def launcher_command(n_gpus, port, bench_args, python=None, script=None):
    """argv of the child that runs N ranks of this script: one process per GPU under torch.distributed.run."""
    return [python or sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_gpus}",
            "--master-addr", "127.0.0.1", "--master-port", str(port), script or os.path.abspath(__file__)] + list(bench_args)


def launcher_env(base):
    """Environment of the child: the caller's, plus what multi-process GPU work needs on this pool."""
    env = dict(base)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")         # dmabuf IPC (RCCL across processes)
    env["SIR_BENCH_LAUNCHED_BY"] = "bench.py"
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)                                      # torch.distributed.run sets them per rank
    return env


def free_port():
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def pick_json_line(lines):
    """The last line that is a JSON object carrying "metric" (rank 0's result)."""
    for line in reversed(lines):
        line = line.strip()
        if line.startswith("{"):
            try:
                d = json.loads(line)
            except ValueError:
                continue
            if isinstance(d, dict) and "metric" in d:
                return line
    return None


def visible_gpu_count(kfd_nodes="/sys/class/kfd/kfd/topology/nodes", env=None):
    """GPUs this process could use, counted WITHOUT touching HIP: KFD topology nodes with a non-zero simd_count, cut down
    by HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES / CUDA_VISIBLE_DEVICES when one is set.  (torch.cuda.device_count()
    falls back to hipGetDeviceCount when amdsmi is not importable, which initialises the runtime in the launcher parent.)
    0 when there is no KFD topology at all (no amdgpu driver: no GPU); None when it exists but cannot be read: the caller
    then skips the pre-check and lets the ranks fail."""
    env = os.environ if env is None else env
    if not os.path.isdir(kfd_nodes):
        return 0
    try:
        n = 0
        for node in sorted(os.listdir(kfd_nodes)):
            with open(os.path.join(kfd_nodes, node, "properties")) as f:
                for line in f:
                    k, _, v = line.partition(" ")
                    if k == "simd_count" and int(v) > 0:
                        n += 1
    except (OSError, ValueError):
        return None
    for var in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        if env.get(var, "") != "":
            n = min(n, len([x for x in env[var].split(",") if x.strip() != ""]))
    return n


def launch_ranks(n_gpus, bench_args):
    """Parent of an N-rank run.  No HIP call is made here (GPUs are counted from the KFD topology in sysfs)."""
    share = os.environ.get("SIR_BENCH_SHARE_GPU", "0") == "1"
    ndev = visible_gpu_count()
    if not share and ndev is not None and ndev < n_gpus:
        print(f"bench.py: --gpus {n_gpus} but only {ndev} GPU(s) are visible (SIR_BENCH_SHARE_GPU=1 rehearses N ranks "
              "on one GPU over gloo)", file=sys.stderr)
        return 2
    cmd = launcher_command(n_gpus, free_port(), bench_args)
    log("launching " + " ".join(cmd))
    proc = subprocess.Popen(cmd, env=launcher_env(os.environ), stdout=subprocess.PIPE, text=True)
    lines = [ln for ln in proc.stdout]
    rc = proc.wait()
    result = pick_json_line(lines)
    for ln in lines:
        if ln.strip() != (result or "").strip():
            sys.stderr.write(ln)
    if result is None:
        print(f"bench.py: the {n_gpus}-rank run printed no result line (exit code {rc})", file=sys.stderr)
        return rc or 1
    print(result, flush=True)
    return rc


def host_cpu_share(cap=16):
    """Threads the CPU leg may really use: min(affinity mask, cgroup CPU quota, cap).  The GPU box
    exposes every host core in the affinity mask but grants a share of them (16 per GPU); running
    hundreds of OpenMP threads against that quota would stall instead of measuring."""
    from sir_amd.dist_utils import host_cpu_share as share
    return max(1, min(share(cap), int(os.environ.get("SIR_BENCH_CPU_THREADS", cap))))


def host_cpu_info():
    """What `cores` was derived from (VERDICT r3 bench hygiene): CPU model, logical CPUs, affinity-mask size, cgroup quota."""
    info = {"os_cpu_count": os.cpu_count(), "cpu_model": None, "affinity_cpus": None, "cgroup_quota_cpus": None}
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    info["cpu_model"] = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    try:
        info["affinity_cpus"] = len(os.sched_getaffinity(0))
    except Exception:
        pass
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()[:2]
        info["cgroup_quota_cpus"] = None if quota == "max" else round(int(quota) / int(period), 2)
    except Exception:
        pass
    return info


def pmc_traffic(kernel):
    """(HBM bytes per launch of `kernel`, source) from the newest COMMITTED rocprofv3 --pmc pass
    (profiles/*/pmc_traffic.json, written by devtools/gpu_pmc.sh + profiles/pmc_to_traffic.py) -- not measured in
    this run, and labelled so -- or (None, None) when no measurement is on file."""
    try:
        import glob
        files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*", "pmc_traffic.json")))
        if not files:
            return None, None
        with open(files[-1]) as f:
            v = (json.load(f).get(kernel) or {}).get("hbm_bytes_per_launch")
        return v, f"{os.path.relpath(files[-1], ROOT)} (committed rocprofv3 --pmc pass, not measured in this run)"
    except Exception:
        return None, None


def dump_outputs(out_dir, arrays, limit, suffix=""):
    """Write `arrays` (name -> tensor, first axis = utterance) as <out_dir>/<name><suffix>.npy: float32 stays float32,
    any other dtype becomes float64.  When the files would exceed `limit` bytes, every array keeps the same fixed,
    seeded sample of utterances (ascending), and their indices are written as sample_rows<suffix>.npy.  Returns the paths."""
    import numpy as np
    arrs = {}
    for name, t in arrays.items():
        a = t.detach().cpu().numpy()
        arrs[name] = a if a.dtype == np.float32 else a.astype(np.float64)
    n = len(next(iter(arrs.values())))
    header = 128                                               # .npy header of a version 1.0 file
    if sum(a.nbytes + header for a in arrs.values()) > limit:
        per_row = sum(a.nbytes // n for a in arrs.values()) + 8
        keep = (limit - header * (len(arrs) + 1)) // per_row
        if keep < 1:
            raise ValueError(f"--dump-outputs: {limit} bytes cannot hold one utterance's outputs")
        rows = np.sort(np.random.default_rng(0).choice(n, size=min(n, keep), replace=False))
        arrs = {name: a[rows] for name, a in arrs.items()}
        arrs["sample_rows"] = rows.astype(np.float64)
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    for name, a in arrs.items():
        paths.append(os.path.join(out_dir, f"{name}{suffix}.npy"))
        np.save(paths[-1], np.ascontiguousarray(a))
    return paths


def device_clips(n, length, seed, device):
    """Synthetic clips generated on the device: 0.1*N(0,1) + A*sin(2*pi*f*n/16000), clamped."""
    g = torch.Generator(device=device).manual_seed(seed)
    x = 0.1 * torch.randn(n, length, generator=g, device=device)
    f = 100.0 + 3900.0 * torch.rand(n, 1, generator=g, device=device)
    a = 0.05 + 0.45 * torch.rand(n, 1, generator=g, device=device)
    t = torch.arange(length, dtype=torch.float32, device=device).unsqueeze(0)
    x += a * torch.sin(2.0 * torch.pi * f * t / 16000.0)
    return x.clamp_(-1.0, 1.0)


def cpu_baseline(target_seconds=12.0):
    """Reference CPU path restated (oracle/): features one clip at a time
    (precompute_features.py:124-130), then batch-8 forward + argmax (evaluate.py:79-86), 32 clips."""
    from oracle import features_ref, model_ref
    from sir_amd import synth
    clips = synth.synth_clips(32, CLIP_LEN, seed=1234)
    sd = synth.synth_state_dict(NUM_CLASSES, seed=0)

    fast = model_ref.FastRef(sd)          # torch's fused CPU kernels (nn.GRU, F.batch_norm), as the reference runs

    def one_pass():
        feats = [features_ref.pad_or_trim(features_ref.extract_features_f32(c)) for c in clips]
        preds = []
        for i in range(0, 32, 8):
            preds.append(fast(torch.stack(feats[i:i + 8])).argmax(1))
        return torch.cat(preds)

    def timed(threads):
        torch.set_num_threads(threads)
        one_pass()
        t0 = time.perf_counter()
        one_pass()
        dt = time.perf_counter() - t0
        reps = max(1, min(50, int(target_seconds / 2 / max(dt, 1e-3))))
        t0 = time.perf_counter()
        for _ in range(reps):
            pred = one_pass()
        return 32 * reps / (time.perf_counter() - t0), reps, pred

    cores = host_cpu_share()
    log(f"cpu_baseline: timing the oracle path on {cores} host threads ...")
    all_rate, reps, pred = timed(cores)
    log(f"cpu_baseline: {all_rate:.1f} utt/s on {cores} threads; timing 1 thread ...")
    one_rate, _, _ = timed(1)
    log(f"cpu_baseline: {one_rate:.1f} utt/s on 1 thread")
    torch.set_num_threads(cores)
    return {"value": round(all_rate, 2), "unit": "utterances/s", "cores": cores, "kind": "port",
            "sample": f"{reps} x (32 synthetic 3 s clips: torch.stft features one clip at a time + batch-8 "
                      f"fp32 forward + argmax), oracle/ restatement of the reference CPU path",
            "single_thread_value": round(one_rate, 2),
            "host": dict(host_cpu_info(), cores_rule="min(affinity mask, cgroup CPU quota, 16): the box grants 16 CPUs per GPU")}, pred


def cpu_train_baseline(cores, target_seconds=8.0):
    """Reference CPU training step restated (train.py:90-107 on stock torch.nn layers, oracle.TrainRef):
    zero_grad, forward, CE, backward, Adam(lr 5e-5, wd 1e-4) on cached features [batch, 64, 200]."""
    from oracle import model_ref
    from sir_amd import synth
    torch.set_num_threads(cores)
    out = {}
    for batch in (8, 256):
        m = model_ref.TrainRef(synth.synth_state_dict(NUM_CLASSES, seed=0), NUM_CLASSES).train()
        opt = torch.optim.Adam(m.parameters(), lr=5e-5, weight_decay=1e-4)
        x = synth.synth_features(batch, 200, seed=7)
        y = synth.synth_labels(batch, NUM_CLASSES, seed=5)

        def step():
            opt.zero_grad(set_to_none=True)
            loss = torch.nn.functional.cross_entropy(m(x), y)
            loss.backward()
            opt.step()
            return loss.item()

        step()
        t0 = time.perf_counter()
        step()
        dt = time.perf_counter() - t0
        reps = max(1, min(30, int(target_seconds / 2 / max(dt, 1e-3))))
        t0 = time.perf_counter()
        for _ in range(reps):
            step()
        out[batch] = (batch * reps / (time.perf_counter() - t0), reps)
        log(f"cpu_train_baseline: batch {batch}: {out[batch][0]:.1f} utt/s ({reps} steps, {cores} threads)")
    best = max(out[8][0], out[256][0])                      # the faster CPU configuration is the baseline
    return {"value": round(best, 2), "unit": "utterances/s", "cores": cores, "kind": "port",
            "sample": f"{out[256][1]} training steps at batch 256 and {out[8][1]} at batch 8 on cached features (value = the "
                      "faster of the two): stock torch.nn layers + CE + backward + Adam, oracle/ restatement of train.py:90-107",
            "batch8_value": round(out[8][0], 2), "batch256_value": round(out[256][0], 2)}


def mfma_roofline(kernel, avg_ms, launches, batch=BATCH):
    """roofline block of one matrix-core kernel from its average launch duration."""
    flops = FLOPS_PER_UTT[kernel] * batch
    achieved = flops / (avg_ms * 1e-3) / 1e12
    x6 = kernel in F16X3_KERNELS
    peak = PEAK_F16X3_TFLOPS if x6 else PEAK_F32_MFMA_TFLOPS
    traffic, source = pmc_traffic(kernel)
    out = {"kernel": kernel, "bound": "mfma", "achieved": round(achieved, 3), "peak": round(peak, 1), "unit": "TFLOP/s",
           "frac": round(achieved / peak, 4), "traffic": traffic, "traffic_source": source,
           "avg_launch_ms": round(avg_ms, 5), "launches": launches, "flops_per_launch": flops,
           "mfma_path": ("f16x3: fp32 product = 3 fp16 MFMA products (two-way fp16 split, residual scaled by 2^11), f32 accumulate; "
                         "peak = 2500/3 algorithmic TFLOP/s; executed fp16 MFMA rate = 3 x achieved.  Rounds 1-3 ran bf16x6 "
                         "(peak 2500/6): the same TFLOP/s was twice the fraction there") if x6 else "v_mfma_f32_32x32x2_f32",
           "fp32_mfma_peak": PEAK_F32_MFMA_TFLOPS}
    if kernel in WINOGRAD_KERNELS:
        out["algorithm"] = ("Winograd F(2x2,3x3): flops_per_launch counts the DIRECT convolution (the algorithmic work); the "
                            "kernel executes 16/36 of its products, i.e. executed fp16 MFMA rate = 3 x 16/36 x achieved")
    return out


class GpuSensors:
    """Package power (W) and shader clock (MHz) of one GPU read from the amdgpu hwmon files in sysfs (no HIP / SMI call, no
    child process), sampled by a background thread while a region runs."""

    def __init__(self, index=0, period=0.25):
        import glob
        self.period = period
        self.power_file = self.sclk_file = None
        self.how = None
        hw = None
        # the card of THIS process: by PCI address (sysfs lists every GPU of the host, the process sees one), else by position
        try:
            pr = torch.cuda.get_device_properties(index)
            bdf = f"{getattr(pr, 'pci_domain_id', 0):04x}:{pr.pci_bus_id:02x}:{pr.pci_device_id:02x}.0"
            cand = sorted(glob.glob(f"/sys/bus/pci/devices/{bdf}/hwmon/hwmon*"))
            if cand:
                hw, self.how = cand[0], f"amdgpu hwmon (sysfs) of PCI device {bdf}"
        except Exception:
            pass
        if hw is None:
            cards = sorted(glob.glob("/sys/class/drm/card*/device/hwmon/hwmon*"))
            cards = [c for c in cards if os.path.exists(os.path.join(c, "power1_average")) or os.path.exists(os.path.join(c, "power1_input"))]
            if index < len(cards):
                hw, self.how = cards[index], f"amdgpu hwmon (sysfs), card position {index} (PCI address not available: may be another GPU of the host)"
        if hw is not None:
            for name in ("power1_average", "power1_input"):
                f = os.path.join(hw, name)
                if os.path.exists(f):
                    self.power_file = f
                    break
            f = os.path.join(hw, "freq1_input")
            self.sclk_file = f if os.path.exists(f) else None
        self.samples = []
        self._stop = None

    @staticmethod
    def _read(path, scale):
        try:
            with open(path) as f:
                return int(f.read().strip()) * scale
        except (OSError, ValueError):
            return None

    def __enter__(self):
        import threading
        self._stop = threading.Event()

        def run():
            while not self._stop.is_set():
                self.samples.append((self._read(self.power_file, 1e-6) if self.power_file else None,
                                     self._read(self.sclk_file, 1e-6) if self.sclk_file else None))
                self._stop.wait(self.period)
        self._thread = threading.Thread(target=run, daemon=True)
        self._thread.start()
        return self

    def __exit__(self, *exc):
        self._stop.set()
        self._thread.join()

    def summary(self):
        out = {"samples": len(self.samples), "source": self.how if self.power_file or self.sclk_file else None}
        for i, key in enumerate(("power_W", "sclk_MHz")):
            v = [s[i] for s in self.samples if s[i] is not None]
            out[key] = {"mean": round(sum(v) / len(v), 1), "max": round(max(v), 1), "min": round(min(v), 1)} if v else None
        return out


class _TimedIter:
    """Wraps a batch iterable: time of the first batch handed over and the clips it held (for a steady-state rate that leaves
    the DataLoader's worker start-up out)."""

    def __init__(self, it):
        self.it, self.t_first, self.n_first, self.n, self.wait_s = it, None, 0, 0, 0.0

    def __iter__(self):
        it = iter(self.it)
        while True:
            t0 = time.perf_counter()
            try:
                item = next(it)
            except StopIteration:
                return
            t1 = time.perf_counter()
            self.wait_s += t1 - t0                       # time the consumer spent waiting for the source to hand over a batch
            k = int(item[0].size(0)) if item[0] is not None else 0
            if self.t_first is None:
                self.t_first, self.n_first = t1, k
            self.n += k
            yield item


def dropin_epoch_leg(model, opt, fz, dev, step_rate, n_clips, batch=BATCH, workers=8):
    """BASELINE configs[2] names `scripts/train.py drop-in, batch=256`: one EPOCH through the reference-shaped entry points over
    a synthetic split of `n_clips` 3 s clips, per route, as utterances/s and as a fraction of the bare step rate (`train.value`):
      dataloader        train_epoch() (train.py:72-118) over FSCIntentDataset + DataLoader(batch 256, num_workers 8, pin_memory)
                        + collate_fn on a feature cache in the reference's file format (train.py:203-219, dataset.py:78-115)
      dataloader_forkserver  the same dataset through the DataLoader as train() builds it with `hbm_feature_cache: false`: fork-server
                        workers (persistent), pin_memory=False, batches through train_epoch's persistent pinned ring (HostStager)
      hbm_feature_store the same cache staged once in HBM (sir_amd/feature_store.py), train_epoch() over its batches: train()'s
                        default route
      waveform_store    train_epoch_waveforms() over WaveformStore on the same clips (`fused_features: true`)
    The split (clips, features, cache file, CSV) is built on the spot; building it is not timed."""
    import shutil
    import tempfile
    import pandas as pd
    from torch.utils.data import DataLoader
    from sir_amd.feature_store import FeatureStore
    from sir_amd.scripts import train as tr
    from sir_amd.scripts.dataset import FSCIntentDataset
    from sir_amd.waveform_store import WaveformStore
    tmp = tempfile.mkdtemp(prefix="sir_dropin_")
    from sir_amd.dist_utils import limit_host_threads
    host_threads = limit_host_threads(reserve=workers)        # as train() does: torch's OpenMP pool inside the CPU quota
    try:
        t_frames = 1 + CLIP_LEN // 512
        pcm = torch.empty((n_clips, CLIP_LEN), dtype=torch.int16, device=dev)
        host_feats = torch.empty((n_clips, 64, t_frames), dtype=torch.float32)
        lengths = torch.full((batch,), CLIP_LEN, dtype=torch.int32, device=dev)
        for start in range(0, n_clips, batch):
            k = min(batch, n_clips - start)
            clips = device_clips(k, CLIP_LEN, 99000 + start, dev)
            pcm[start:start + k] = (clips * 32767.0).round().to(torch.int16)
            host_feats[start:start + k] = fz(pcm[start:start + k], lengths[:k], t_pad=T_PAD)[:, :, :t_frames].cpu()
        labels = torch.randint(0, NUM_CLASSES, (n_clips,), generator=torch.Generator().manual_seed(7))
        names = [f"intent_{i:02d}" for i in range(NUM_CLASSES)]
        paths = [os.path.join(tmp, "wav", f"clip{i:06d}.wav") for i in range(n_clips)]       # never opened: every clip is cached
        csv = os.path.join(tmp, "train_data.csv")
        pd.DataFrame({"path": paths, "label": [names[int(v)] for v in labels]}).to_csv(csv, index=False)
        lm = os.path.join(tmp, "label_map.json")
        with open(lm, "w") as f:
            json.dump({n: i for i, n in enumerate(names)}, f)
        cache_dir = os.path.join(tmp, "cache")
        os.makedirs(cache_dir)
        torch.save({p: {"features": host_feats[i], "label": names[int(labels[i])]} for i, p in enumerate(paths)},
                   os.path.join(cache_dir, "train_data_features.pt"))
        del host_feats
        crit = torch.nn.CrossEntropyLoss()
        aug_prob = 0.7                                   # configs/config.yaml:39
        model.train()

        def run(make_batches, epoch_fn):
            """two epochs, the second one reported: (utt/s over the whole call, steady utt/s after the first batch, seconds)"""
            best = None
            for e in range(2):
                it = _TimedIter(make_batches(e))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                epoch_fn(it)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                best = {"utts_per_s": round(it.n / (t1 - t0), 1), "epoch_s": round(t1 - t0, 4), "waiting_for_batches_s": round(it.wait_s, 4),
                        "steady_utts_per_s": round((it.n - it.n_first) / max(t1 - it.t_first, 1e-9), 1),
                        "first_batch_after_s": round(it.t_first - t0, 4), "clips": it.n}
            best["frac_of_step_rate"] = round(best["utts_per_s"] / step_rate, 4)
            best["steady_frac_of_step_rate"] = round(best["steady_utts_per_s"] / step_rate, 4)
            return best

        out = {"clips": n_clips, "batch": batch, "num_workers": workers, "augment_prob": aug_prob, "step_rate": step_rate,
               "main_process_torch_threads": host_threads,
               "note": "fractions are of `train.value` (the bare step on HBM-resident clips); `steady_*` leaves out the time to the "
                       "first batch (DataLoader worker start-up, paid every epoch as in the reference: no persistent workers)"}
        # ---- route 1: the reference's own shape ----
        t0 = time.perf_counter()
        ds = FSCIntentDataset(csv, lm, is_training=True, augment_prob=aug_prob, cache_dir=cache_dir)
        load_s = time.perf_counter() - t0

        def loader(_e):
            return DataLoader(ds, batch_size=batch, shuffle=True, num_workers=workers, collate_fn=tr.collate_fn, pin_memory=True)

        lo = _TimedIter(loader(0))
        t0 = time.perf_counter()
        for mel, lab in lo:                              # loader alone: what the host side can deliver
            mel = mel.to(dev, non_blocking=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        r = run(loader, lambda it: tr.train_epoch(model, it, opt, crit, dev))
        r["loader_only_utts_per_s"] = round(lo.n / (t1 - t0), 1)
        r["loader_only_steady_utts_per_s"] = round((lo.n - lo.n_first) / max(t1 - lo.t_first, 1e-9), 1)
        r["cache_load_s"] = round(load_s, 3)
        r["limit"] = ("host batch assembly (worker __getitem__ + collate_fn + pinned copy + H2D): "
                      f"{r['waiting_for_batches_s']:.2f} s of the {r['epoch_s']:.2f} s epoch are spent waiting for the DataLoader to hand over a "
                      f"batch; the loader alone, with an idle main thread, delivers {r['loader_only_steady_utts_per_s']:.0f} utt/s"
                      if r["waiting_for_batches_s"] > 0.5 * r["epoch_s"] else "the GPU step")
        r["limit"] = ("the loader's own pinning: " + r["limit"]) if r["limit"] != "the GPU step" else (
            "GPU submission from a process with FORKED children, not batch assembly: the step loop waits for batches only "
            f"{r['waiting_for_batches_s']:.2f} s of {r['epoch_s']:.2f} s; while the DataLoader's forked workers live, every kernel launch "
            "of the parent is ~50x slower (devtools/dataloader_probe.py, profiles/r04/dataloader_probe.txt: 3 k utt/s with fork, 34 k "
            "with fork-server workers, any consumer that launches a kernel)")
        out["dataloader"] = r
        # the same route as train() builds it when `hbm_feature_cache: false` (scripts/train.py::loader_kwargs): workers from a fork
        # server (they do not inherit the HIP-initialised parent), kept alive across the epochs, pin_memory=False, batches staged by
        # train_epoch's own persistent pinned ring (HostStager)
        fs_loader = DataLoader(ds, batch_size=batch, shuffle=True, collate_fn=tr.collate_fn, **tr.loader_kwargs(workers))
        r = run(lambda _e: fs_loader, lambda it: tr.train_epoch(model, it, opt, crit, dev))
        del fs_loader
        r["limit"] = ("host batch assembly (worker __getitem__ + collate_fn + shared-memory hand-over): "
                      f"{r['waiting_for_batches_s']:.2f} s of the {r['epoch_s']:.2f} s epoch are spent waiting for the DataLoader"
                      if r["waiting_for_batches_s"] > 0.4 * r["epoch_s"] else "the step loop's own host work + the GPU step")
        out["dataloader_forkserver"] = r
        del ds
        # ---- route 2: the cache staged in HBM (train()'s default) ----
        t0 = time.perf_counter()
        store = FeatureStore(csv, lm, dev, cache_dir=cache_dir)
        stage_s = time.perf_counter() - t0
        r = run(lambda e: store.epoch_batches(batch, shuffle=True, seed=0, epoch=e, augment_prob=aug_prob),
                lambda it: tr.train_epoch(model, it, opt, crit, dev))
        r["stage_s"] = round(stage_s, 3)
        r["limit"] = "the GPU step (one gather launch per batch, no host data path)"
        out["hbm_feature_store"] = r
        del store
        # ---- route 3: raw waveforms in HBM, features inside the step ----
        wstore = WaveformStore.from_tensors(pcm, torch.full((n_clips,), CLIP_LEN, dtype=torch.int32, device=dev), labels.to(dev))
        cfg = {"augment_prob": aug_prob}
        r = run(lambda e: wstore.epoch_batches(batch, shuffle=True, seed=0, epoch=e),
                lambda it: tr.train_epoch_waveforms(model, it, opt, crit, dev, t_pad=T_PAD,
                                                    augment=tr.make_waveform_augment(cfg, seed=0, epoch=0)))
        r["limit"] = "the GPU step (feature kernel one batch ahead on a side stream)"
        out["waveform_store"] = r
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5, help="timed regions of --steps steps each; the median is reported")
    ap.add_argument("--full", action="store_true",
                    help="after the timed regions, also run the legs that take runs of their own: single-stream regions and "
                         "roofline, sustained region, training legs, CPU baselines and parity (the --no-* switches below "
                         "and --train-steps, --dropin-clips, --sustain-seconds apply to them)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-train", action="store_true", help="skip the training-step legs")
    ap.add_argument("--augment", dest="augment", action="store_true", default=True,
                    help="also time the training step with fused time-shift + noise + SpecAugment masks (default on)")
    ap.add_argument("--no-augment", dest="augment", action="store_false")
    ap.add_argument("--no-host-feed", action="store_true", help="skip the training leg fed from pinned host memory")
    ap.add_argument("--no-dropin", action="store_true", help="N = 1 only: skip the `dropin_epoch` block (train_epoch() over the "
                    "reference-shaped DataLoader route, the HBM feature store and the waveform store on a synthetic 16 384-clip split)")
    ap.add_argument("--dropin-clips", type=int, default=int(os.environ.get("SIR_BENCH_DROPIN_CLIPS", "16384")))
    ap.add_argument("--train-steps", type=int, default=20)
    ap.add_argument("--sustain-seconds", type=float, default=6.0,
                    help="one extra region of pipelined inference steps of at least this many seconds (0 = skip): long enough "
                         "for a 5-second SMI sampler to see the load; reports throughput, package power and sclk")
    ap.add_argument("--no-dist-leg", action="store_true",
                    help="N = 1 only: skip the training leg that runs the RCCL gradient exchange in a one-rank nccl group")
    ap.add_argument("--streams", type=int, default=int(os.environ.get("SIR_BENCH_STREAMS", "2")),
                    help="HIP streams the inference batches alternate over (each with its own buffers/workspace)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed regions, write what the last timed inference step returned (features, logits, "
                         "predictions) as DIR/<name>.npy (DIR/<name>_rank<r>.npy with N > 1), float32 / float64, at most "
                         "64 MB in all; the inputs depend only on the arguments")
    args = ap.parse_args()
    if args.steps < 1 or args.repeats < 1:
        ap.error("--steps and --repeats must be at least 1")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args.gpus, sys.argv[1:]))       # parent: launcher only, before any GPU call

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: refusing to run a different job than the one asked for",
              file=sys.stderr)
        sys.exit(2)
    # SIR_BENCH_SHARE_GPU=1 (rehearsal on a one-GPU box): every rank uses cuda:0 and the gloo backend, to exercise
    # the multi-rank code path; real runs use one GPU per rank and RCCL ("nccl")
    share_gpu = os.environ.get("SIR_BENCH_SHARE_GPU", "0") == "1"
    batch = BATCH
    if share_gpu:
        local_rank = 0
        # N ranks on ONE GPU is a rehearsal of the code path, not a measurement: the GRU recurrences are cluster kernels
        # whose workgroups own a whole CU each (128 / 256 of them per launch at batch 256), and launches of SEVERAL
        # processes cannot be chained against each other, so the ranks get a batch whose clusters all fit side by side
        batch = max(16, BATCH // (2 * world))
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        if share_gpu:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)

    from sir_amd import _native, ops, synth
    from sir_amd.featurizer import get_featurizer
    from sir_amd.models.models import CNNAudioGRU
    if not os.path.exists(_native.LIB_PATH):
        if rank == 0:
            _native.build()
        if dist is not None:
            dist.barrier()
    lib = _native.lib()

    # what the process group really is (so that "RCCL saw N ranks" is checkable from the JSON line)
    my_dev = f"rank{rank}:cuda:{local_rank}:{torch.cuda.get_device_name(local_rank)}"
    try:
        my_dev += ":" + str(torch.cuda.get_device_properties(local_rank).uuid)
    except Exception:
        pass
    if dist is not None:
        devices = [None] * world
        dist.all_gather_object(devices, my_dev)
        dist_info = {"world_size": dist.get_world_size(), "backend": dist.get_backend(), "devices": devices,
                     "launcher": os.environ.get("SIR_BENCH_LAUNCHED_BY", "external")}
    else:
        dist_info = {"world_size": 1, "backend": None, "devices": [my_dev], "launcher": None}

    sd = synth.synth_state_dict(NUM_CLASSES, seed=0)
    model = CNNAudioGRU(NUM_CLASSES)
    model.load_state_dict(sd)
    model = model.to(dev).eval()
    fz = get_featurizer()
    pool = [device_clips(batch, CLIP_LEN, 1234 + 1000 * rank + i, dev) for i in range(N_POOL)]
    lengths = torch.full((batch,), CLIP_LEN, dtype=torch.int32, device=dev)
    last = [None]                # (slot, logits, predictions) of the latest inference step
    # batch pipelining INSIDE the library (sir_pipeline, include/sir_hip.h; sir_amd/pipeline.py wraps it): this process
    # stays on ONE stream; the library alternates consecutive batches over `--streams` streams of its own, each with its
    # own feature buffer and model workspace (weights shared), so that the latency-bound GRU recurrence of one batch
    # overlaps the matrix-core-bound convolutions of the next
    from sir_amd.pipeline import BatchPipeline
    ns = max(1, args.streams)
    pipe = BatchPipeline(model, n_streams=ns)
    feats = [torch.empty(batch, 64, T_PAD, device=dev) for _ in range(ns)]

    def step(i):
        k = pipe.slot(i)
        pipe.features(i, pool[i % N_POOL], lengths, t_pad=T_PAD, out=feats[k])
        last[0] = (k,) + pipe.infer(i, feats[k])

    nk = lib.sir_profile_kernel_count()
    names = [lib.sir_profile_kernel_name(i).decode() for i in range(nk)]

    def collect():
        ms = (C.c_double * nk)()
        cnt = (C.c_int64 * nk)()
        _native.check(lib.sir_profile_collect(fz.handle, ms, cnt, nk), "sir_profile_collect")
        return {names[i]: (ms[i] / cnt[i] if cnt[i] else 0.0) for i in range(nk)}, {names[i]: cnt[i] for i in range(nk)}

    def timed_regions(fn, steps, repeats):
        """`repeats` regions of exactly `steps` steps: barrier + synchronize on both sides, max over ranks."""
        out = []
        for r in range(repeats):
            if dist is not None:
                dist.barrier()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps):
                fn(r * steps + i)
            torch.cuda.synchronize()
            if dist is not None:
                dist.barrier()
            el = time.perf_counter() - t0
            if dist is not None:
                tm = torch.tensor([el], dtype=torch.float64, device=dev)
                dist.all_reduce(tm, op=dist.ReduceOp.MAX)
                el = float(tm.item())
            out.append(el)
        return out

    def region_stats(times, steps):
        ms = sorted(t / steps * 1e3 for t in times)
        return {"repeats": len(ms), "steps_per_region": steps, "median_ms_per_step": round(statistics.median(ms), 4),
                "min_ms_per_step": round(ms[0], 4), "max_ms_per_step": round(ms[-1], 4)}

    for i in range(args.warmup):
        step(i)
    torch.cuda.synchronize()
    if rank == 0:
        log(f"warm-up done ({args.warmup} steps); profiling 5 steps per kernel")

    # untimed: per-kernel HIP-event times of a few steps -> pick the dominant kernel
    lib.sir_profile_enable(fz.handle, 1, -1)
    for i in range(5):
        step(i)
        torch.cuda.synchronize()          # one batch at a time: per-kernel times without cross-stream overlap
    kernel_ms, _ = collect()
    infer_names = names[:names.index("train_weight_prep")]
    dominant = max(infer_names, key=lambda k: kernel_ms[k])
    lib.sir_profile_enable(fz.handle, 2, names.index(dominant))

    # timed regions: exactly K steps each; the dominant kernel is bracketed by a HIP event pair on its own stream.  A plain
    # run reports no roofline, but keeps the pass above and the event pair so that its timed steps are the --full run's
    times = timed_regions(step, args.steps, args.repeats)
    elapsed = statistics.median(times)
    if rank == 0:
        log(f"timed {args.repeats} x {args.steps} steps: median {elapsed:.4f} s")
    dom_ms, dom_cnt = collect()
    if args.dump_outputs:
        # the last timed step (index repeats * steps - 1); its slot's buffers are reused by the legs below
        k, logits, pred = last[0]
        paths = dump_outputs(args.dump_outputs, {"features": feats[k], "logits": logits, "predictions": pred},
                             DUMP_LIMIT_BYTES // world, f"_rank{rank}" if world > 1 else "")
        log(f"rank {rank}: outputs of timed step {args.repeats * args.steps - 1} written: {' '.join(paths)}")
    # reference leg: the same regions strictly serial (sir_pipeline with one slot = the caller's stream), dominant kernel
    # timed in isolation.  (A single batch cannot be made to overlap with itself: all its utterances already advance in
    # parallel inside the recurrence, so any split only lengthens the dependent chain -- DESIGN.md section 4.)
    single = None
    if args.full and ns > 1:
        pipe1 = BatchPipeline(model, n_streams=1)

        def step1(i):
            fz(pool[i % N_POOL], lengths, t_pad=T_PAD, out=feats[0])
            pipe1.infer(i, feats[0])
        for i in range(5):
            step1(i)
        torch.cuda.synchronize()
        collect()
        t1 = timed_regions(step1, args.steps, args.repeats)
        el1 = statistics.median(t1)
        iso_ms, iso_cnt = collect()
        single = {"value": round(batch * world * args.steps / el1, 1), "ms_per_step": round(el1 / args.steps * 1e3, 4),
                  "timed_regions": region_stats(t1, args.steps),
                  "dominant_avg_launch_ms": round(iso_ms[dominant], 5), "dominant_launches": iso_cnt[dominant]}
    lib.sir_profile_enable(fz.handle, 0, -1)

    # one long region of the SAME pipelined steps: >= --sustain-seconds of back-to-back batches so that
    # an external SMI sampler sees the load, with package power / sclk sampled from sysfs beside it (the "matrix-core
    # kernels sit at the power cap" claim of DESIGN.md section 4 then shows up in this line)
    sustained = None
    if args.full and args.sustain_seconds > 0:
        chunk = 256
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        with GpuSensors(local_rank) as sens:
            t0 = time.perf_counter()
            n_done = 0
            while True:
                for i in range(chunk):
                    step(n_done + i)
                n_done += chunk
                torch.cuda.synchronize()
                if time.perf_counter() - t0 >= args.sustain_seconds:
                    break
            s_el = time.perf_counter() - t0
        sustained = dict(value=round(batch * n_done / s_el, 1), unit="utterances/s (this rank)", steps=n_done,
                         seconds=round(s_el, 3), ms_per_step=round(s_el / n_done * 1e3, 4),
                         note=f"pipelined inference steps back to back, host sync every {chunk} steps", **sens.summary())
        if rank == 0:
            log(f"sustained region: {sustained['value']} utt/s over {s_el:.1f} s, sensors {sens.summary()}")

    # further legs (reported inside the same JSON line): the training step of BASELINE configs[2]/[3]/[4]
    # -- fused HIP features + forward/backward + Adam at per-GPU batch 256; with N > 1 each step
    # ends in the RCCL all-reduce (mean) of the flat 13 MB gradient buffer (two buckets, overlapped).
    gpu_pred32 = None
    cpu_leg = args.full and world == 1 and not args.no_cpu_baseline
    if rank == 0 and cpu_leg:
        # predictions of the sample the CPU baseline runs, taken before the training leg moves the weights
        _, gpu_pred32 = model.predict(fz(synth.synth_clips(32, CLIP_LEN, seed=1234).to(dev)))
        gpu_pred32 = gpu_pred32.cpu()
    train_info = train_aug_info = None
    if args.full and not args.no_train:
        from sir_amd import train_ops
        from sir_amd.optim import FusedAdam
        from sir_amd.scripts import augment as aug
        import random
        model.train()
        opt = FusedAdam(model.parameters(), lr=5e-5, weight_decay=1e-4)
        labels = torch.randint(0, NUM_CLASSES, (batch,), device=dev)
        host_lengths = [CLIP_LEN] * batch
        rng = random.Random(4321 + rank)

        def tstep(i, augment=False):
            kw = {}
            if augment:
                # BASELINE configs[4]: shift U(-0.1, 0.1) * L and sigma U(1e-3, 1e-2) with the reference's gating
                # (scripts/augment.py:98-135), SpecAugment bands (dataset.py:160-176), all applied inside the feature kernels
                shift, sigma = aug.draw_batch_params(host_lengths, 0.7, rng)
                tm, fm = aug.draw_spec_masks([1 + n // 512 for n in host_lengths], 0.5, rng=rng)
                kw = dict(shift=shift, noise_sigma=sigma, noise_seed=(rank << 32) ^ i, time_mask=tm, freq_mask=fm)
            x = fz(pool[i % N_POOL], lengths, t_pad=T_PAD, out=feats[0], **kw)
            opt.zero_grad(set_to_none=True)
            loss = train_ops.fused_cross_entropy(model(x), labels)
            loss.backward()
            opt.step()

        def train_leg(augment):
            fn = (lambda i: tstep(i, True)) if augment else tstep
            for i in range(5):
                fn(i)
            torch.cuda.synchronize()
            lib.sir_profile_enable(fz.handle, 1, -1)              # untimed: per-kernel times of three steps
            for i in range(3):
                fn(i)
            torch.cuda.synchronize()
            tk_ms, _ = collect()
            tdom = max((k for k in tk_ms if k in FLOPS_PER_UTT and k in BF16X6_KERNELS), key=lambda k: tk_ms[k])
            lib.sir_profile_enable(fz.handle, 2, names.index(tdom))
            tt = timed_regions(fn, args.train_steps, args.repeats)
            td_ms, td_cnt = collect()
            lib.sir_profile_enable(fz.handle, 0, -1)
            t_el = statistics.median(tt)
            ms = t_el / args.train_steps * 1e3
            step_tf = TRAIN_FLOPS_PER_UTT * batch / (ms * 1e-3) / 1e12
            info = {"value": round(batch * world * args.train_steps / t_el, 1), "unit": "utterances/s",
                    "ms_per_step": round(ms, 4), "steps": args.train_steps, "timed_regions": region_stats(tt, args.train_steps),
                    "workload": "waveform batch 256/GPU -> HIP features" +
                                (" with fused time-shift + noise + SpecAugment masks" if augment else "") +
                                " -> forward/backward (dropout 0.5, batch-stat BN; the backward's weight-gradient launches on a second, "
                                "library-owned stream: SIR_BWD_STREAMS) -> Adam(lr 5e-5, wd 1e-4)" +
                                (", RCCL all-reduce of 13 MB grads in two overlapped buckets" if world > 1 else ""),
                    "model_flops_per_utt_fwd_bwd": TRAIN_FLOPS_PER_UTT,
                    "roofline": dict(mfma_roofline(tdom, td_ms[tdom], td_cnt[tdom], batch),
                                     whole_step={"flops_per_step": TRAIN_FLOPS_PER_UTT * batch, "achieved": round(step_tf, 2),
                                                 "peak": round(PEAK_F16X3_TFLOPS, 1), "unit": "TFLOP/s",
                                                 "frac": round(step_tf / PEAK_F16X3_TFLOPS, 4),
                                                 "note": "1.2019 GFLOP/utt (fwd + dgrad + wgrad convention) x 256 / per-GPU step time"}),
                    "kernels_avg_ms": {k: round(v, 5) for k, v in tk_ms.items() if v > 0.0},
                    "kernels_avg_ms_note": "HIP-event times of an untimed pass in which the backward stays on ONE stream (un-overlapped "
                                           "kernel times: their sum exceeds ms_per_step, whose timed regions run the two-stream form)"}
            if rank == 0:
                log(f"train leg (augment={augment}): {info['value']} utt/s")
            return info

        train_info = train_leg(False)
        if args.augment:
            train_aug_info = train_leg(True)
        if world == 1 and not args.no_dist_leg:
            # the REAL collective backend on the one GPU of this box.  A one-rank "nccl" (RCCL) group, and the
            # same training step taking the data-parallel path: async all-reduce of the GRU / head bucket on RCCL's stream beside
            # the conv backward, the conv bucket, the waits and the 1/W scale.  The sum over one rank is the identity, so the
            # difference to `train.value` is the per-step cost of the collective plumbing that every N pays once.
            try:
                import torch.distributed as dist1
                os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
                os.environ.setdefault("MASTER_PORT", str(free_port()))
                dist1.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
                train_ops.FORCE_EXCHANGE = True
                try:
                    leg = train_leg(False)
                    backend = dist1.get_backend()
                finally:
                    train_ops.FORCE_EXCHANGE = False
                    dist1.destroy_process_group()
                train_info["rccl_world1"] = {
                    "value": leg["value"], "unit": "utterances/s", "ms_per_step": leg["ms_per_step"], "backend": backend,
                    "world_size": 1, "timed_regions": leg["timed_regions"],
                    "vs_plain_step": round(leg["ms_per_step"] / train_info["ms_per_step"], 4),
                    "path": "two-bucket overlapped gradient exchange (train_ops._exchange_and_scale) over a one-rank RCCL group"}
            except Exception as e:                       # never lose the bench line to the extra leg
                train_info["rccl_world1"] = {"error": f"{type(e).__name__}: {e}"}
            log(f"train leg over a one-rank nccl group: {train_info['rccl_world1']}")
        if world == 1 and not args.no_host_feed:
            # the same training step fed from HOST memory -- pinned PCM16 batches (24.6 MB each, what a
            # loader would hand over), copied and featurised one batch ahead on a side stream (FeaturePrefetcher) -- so that
            # the PCIe-inclusive rate is a measured number, not an estimate.  Never the headline `value`.
            from sir_amd.pipeline import FeaturePrefetcher
            host_pool = [(p.clamp(-1, 1) * 32767).round().to(torch.int16).cpu().pin_memory() for p in pool[:4]]
            pre = FeaturePrefetcher(t_pad=T_PAD)

            def submit(i):
                with torch.cuda.stream(pre.stream):               # the copy itself runs on the side stream, beside the step
                    w = host_pool[i % len(host_pool)].to(dev, non_blocking=True)
                pre.submit(w, lengths)

            submit(0)

            def hstep(i):
                x = pre.get()
                submit(i + 1)                                  # H2D copy + feature kernel of the next batch, side stream
                opt.zero_grad(set_to_none=True)
                loss = train_ops.fused_cross_entropy(model(x), labels)
                loss.backward()
                opt.step()
                pre.release()

            for i in range(3):
                hstep(i)
            torch.cuda.synchronize()
            ht = timed_regions(hstep, args.train_steps, args.repeats)
            h_el = statistics.median(ht)
            train_info["host_fed"] = {"value": round(batch * args.train_steps / h_el, 1), "unit": "utterances/s",
                                      "ms_per_step": round(h_el / args.train_steps * 1e3, 4),
                                      "timed_regions": region_stats(ht, args.train_steps),
                                      "feed": "pinned host PCM16 [256, 48000] per step (24.6 MB over PCIe) -> H2D on a side stream -> "
                                              "feature kernel one batch ahead (FeaturePrefetcher) -> the same training step",
                                      "h2d_GBs_needed": round(batch * CLIP_LEN * 2 * args.train_steps / h_el / 1e9, 2)}
            if rank == 0:
                log(f"train leg fed from host memory: {train_info['host_fed']['value']} utt/s")
        if world == 1 and not args.no_dropin:
            try:
                train_info["dropin_epoch"] = dropin_epoch_leg(model, opt, fz, dev, train_info["value"], args.dropin_clips, batch)
            except Exception as e:                       # never lose the bench line to the extra block
                train_info["dropin_epoch"] = {"error": f"{type(e).__name__}: {e}"}
            log(f"dropin_epoch: {json.dumps(train_info['dropin_epoch'])}")
        model.eval()
    ops.check_status()                                          # a timed-out GRU recurrence would invalidate every figure

    if rank == 0:
        total_utts = batch * world * args.steps
        value = total_utts / elapsed
        roofline = None
        if args.full:
            d_ms = dom_ms[dominant]
            if dominant in FLOPS_PER_UTT:
                roofline = mfma_roofline(dominant, d_ms, dom_cnt[dominant], batch)
                if single is not None:
                    # with several streams the kernel's launches in the pipelined region share the CUs with the other stream's
                    # kernels (its "duration" then includes co-scheduling); the roofline of the KERNEL is taken from the
                    # single-stream timed leg of this same run (K steps, HIP events on the launch stream), and the pipelined
                    # figures are kept beside it
                    iso = mfma_roofline(dominant, single["dominant_avg_launch_ms"], single["dominant_launches"], batch)
                    iso["pipelined"] = {"streams": ns, "avg_launch_ms": roofline["avg_launch_ms"], "achieved": roofline["achieved"],
                                        "frac": roofline["frac"],
                                        "note": "same kernel inside the multi-stream timed region: it shares the GPU with the other "
                                                "stream's kernels, so its launch duration includes co-scheduling"}
                    iso["measured_in"] = "single-stream timed leg of this run (same K steps, one HIP stream)"
                    roofline = iso
            else:
                achieved = FEATURE_BYTES_PER_UTT * batch / (d_ms * 1e-3) / 1e9
                roofline = {"kernel": dominant, "bound": "hbm", "achieved": round(achieved, 2), "peak": PEAK_HBM_GBS,
                            "unit": "GB/s", "frac": round(achieved / PEAK_HBM_GBS, 4), "traffic": None,
                            "avg_launch_ms": round(d_ms, 5), "launches": dom_cnt[dominant],
                            "bytes_per_launch": FEATURE_BYTES_PER_UTT * batch}
            # the kernel SYMBOL with the largest total time of a step (two launches of one symbol add up), beside the largest single launch
            sym_ms, sym_flops = {}, {}
            for k in infer_names:
                if kernel_ms.get(k, 0.0) > 0.0 and k in KERNEL_SYMBOL:
                    sym_ms[KERNEL_SYMBOL[k]] = sym_ms.get(KERNEL_SYMBOL[k], 0.0) + kernel_ms[k]
                    sym_flops[KERNEL_SYMBOL[k]] = sym_flops.get(KERNEL_SYMBOL[k], 0) + FLOPS_PER_UTT.get(k, 0) * batch
            if sym_ms:
                top = max(sym_ms, key=lambda k: sym_ms[k])
                tf = sym_flops[top] / (sym_ms[top] * 1e-3) / 1e12 if sym_flops[top] else None
                roofline["by_symbol"] = {"symbol": top, "total_ms_per_step": round(sym_ms[top], 5),
                                         "share_of_serial_step": round(sym_ms[top] / sum(sym_ms.values()), 4),
                                         "achieved": round(tf, 3) if tf else None, "peak": round(PEAK_F16X3_TFLOPS, 1), "unit": "TFLOP/s",
                                         "frac": round(tf / PEAK_F16X3_TFLOPS, 4) if tf else None,
                                         "measured_in": "untimed HIP-event pass, one batch at a time (5 steps)"}
        feat_ms = kernel_ms.get("feat_frames", 0.0)      # ONE fused kernel since round 2 (profile id "feat_frames")
        gru = {}
        for k, algo in GRU_ALGO_BYTES.items():
            algo = algo * batch // BATCH
            tr, src = pmc_traffic(k)
            gru[k] = {"avg_ms": round(kernel_ms.get(k, 0.0), 5), "algorithmic_bytes_per_launch": algo, "traffic": tr,
                      "traffic_source": src, "traffic_over_algorithmic": round(tr / algo, 2) if tr else None,
                      "achieved_TFLOPs": round(FLOPS_PER_UTT[k] * batch / (kernel_ms[k] * 1e-3) / 1e12, 2) if kernel_ms.get(k) else None}
        out = {
            "metric": "utterances/sec (16 kHz, 3 s clips), inference: HIP STFT+mel+CNN/BiGRU forward + argmax",
            "value": round(value, 1), "unit": "utterances/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 4), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "timed_regions": region_stats(times, args.steps),
            "config": {"workload": "1xMI355X inference (BASELINE configs[1]): batch=256 synthetic 16 kHz / 3 s clips "
                                   "resident in HBM -> 64-mel log-mel [64,200] -> CNNAudioGRU(31) forward -> argmax",
                       "batch_per_gpu": batch, "clip_samples": CLIP_LEN, "n_mels": 64, "frames": T_PAD,
                       "num_classes": NUM_CLASSES, "parallelism": f"utterance-sharded x{world}, no data-path collective",
                       "streams_per_gpu": ns, "pipelining": "library-owned (sir_pipeline): the caller uses one stream",
                       "share_gpu_rehearsal": share_gpu,
                       "arithmetic": "fp32 accuracy end to end: contractions as f16x3 (two-way fp16 split of both operands -- hi = fp16(x), lo = "
                                     "fp16((x - hi) * 2^11) --, three v_mfma_f32_*_f16 products, f32 accumulation; error vs a float64 product "
                                     "0.45-0.5x bf16x6's on the real GRU operands, profiles/r04/ab_f16x3.txt), the backward under a "
                                     "power-of-two loss scale (exact), everything else fp32 VALU"},
            "dist": dist_info,
            "kernels_avg_ms": {k: round(kernel_ms[k], 5) for k in infer_names if kernel_ms[k] > 0.0},
            "features_stage": {"bound": "hbm", "avg_ms": round(feat_ms, 5),
                               "achieved_GBs": round(FEATURE_BYTES_PER_UTT * batch / (feat_ms * 1e-3) / 1e9, 1) if feat_ms else None,
                               "peak_GBs": PEAK_HBM_GBS, "frac": round(FEATURE_BYTES_PER_UTT * batch / (feat_ms * 1e-3) / 1e9 / PEAK_HBM_GBS, 4) if feat_ms else None,
                               "bytes_per_launch": FEATURE_BYTES_PER_UTT * batch},
            "gru_recurrence": gru,
        }
        if roofline is not None:
            out["roofline"] = roofline
        if single is not None:
            out["single_stream"] = single
        if sustained is not None:
            out["sustained"] = sustained
        if train_info is not None:
            out["train"] = train_info
        if train_aug_info is not None:
            out["train_aug"] = train_aug_info
        if cpu_leg:
            base, cpu_pred = cpu_baseline()
            out["cpu_baseline"] = base
            out["speedup_vs_cpu_all_cores"] = round(value / base["value"], 1)
            # parity flag on the very sample the CPU baseline ran: predicted indices identical
            out["parity"] = {"argmax_identical_on_cpu_sample": bool(torch.equal(gpu_pred32, cpu_pred)),
                             "tolerances": {"features": "|a-b| <= 1e-4*max(1,|b|) on dB and normalised features (north_star 1e-4 rel); "
                                                        "pure-tone clips (> 100 dB dynamic range): 2x the float32 oracle's own error vs "
                                                        "float64, floor 1e-3 dB (tests/test_features_gpu.py) -- looser than 1e-4",
                                            "logits": "<= 2e-5 abs vs the reference's own outputs", "argmax": "identical",
                                            "gradients": "max|a-b| <= 2e-3*rms(b) per tensor (oracle at the device's ReLU/pool decisions)"},
                             "feature_oracle": "parity unpinned by the reference (torchaudio absent, no vectors); cross-checked "
                                               "against transformers.audio_utils.spectrogram (tests/test_oracle_golden.py)"}
            if train_info is not None:
                tb = cpu_train_baseline(base["cores"])
                out["train"]["cpu_baseline"] = tb
                out["train"]["speedup_vs_cpu_all_cores"] = round(train_info["value"] / tb["value"], 1)
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
