"""Drop-in for /root/reference/scripts/train.py: ``collate_fn``, ``train_epoch``, ``validate``,
``train`` with the reference's signatures, YAML keys and checkpoint format, running the step body
(forward, CE loss, backward, Adam) as hand-written HIP kernels on MI355X, plus single-node
data-parallel training (one process per GPU, utterances sharded, one RCCL all-reduce of the flat
gradient buffer per step) which the reference does not have (it pins CUDA_VISIBLE_DEVICES=0,
train.py:17).

Launch:  python -m sir_amd.scripts.train --config cfg.yaml            (1 GPU)
         python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 \
                -m sir_amd.scripts.train --config cfg.yaml             (8 GPUs, per-GPU batch_size)
"""
import argparse
import os

import torch
import torch.nn as nn
import yaml
from torch.utils.data import DataLoader
from tqdm import tqdm

from sir_amd.pipeline import HostStager  # noqa: F401  (bench.py, scripts/evaluate.py and devtools import it from here)

MAX_LENGTH = 200


def load_config(config_path):
    with open(config_path, "r") as f:
        return yaml.safe_load(f)


def collate_fn(batch):
    """(mel, label) items -> ([B,64,200] float32, [B] int64); drops ``None``/empty items, trims or
    zero-pads the time axis to 200, returns (None, None) for an empty batch (train.py:49-70)."""
    mel_specs, labels = [], []
    for mel, label in batch:
        if mel is None or mel.shape[0] == 0 or mel.shape[1] == 0:
            continue
        if mel.size(1) > MAX_LENGTH:
            mel = mel[:, :MAX_LENGTH]
        elif mel.size(1) < MAX_LENGTH:
            mel = torch.nn.functional.pad(mel, (0, MAX_LENGTH - mel.size(1)))
        mel_specs.append(mel)
        labels.append(label)
    if not mel_specs:
        return None, None
    if torch.is_tensor(labels[0]):                         # slot heads: an item's label is int64 [G]
        return torch.stack(mel_specs), torch.stack(labels).to(torch.long)
    return torch.stack(mel_specs), torch.tensor(labels, dtype=torch.long)


def _loss_fn(criterion):
    """The HIP cross-entropy when the criterion is the reference's ``nn.CrossEntropyLoss()`` (mean reduction, no
    weights, default ``ignore_index``, train.py:242) or that with ``label_smoothing=eps`` (``sir_ce_loss_soft``); any
    other criterion is called as is."""
    import functools
    from sir_amd import train_ops
    if (isinstance(criterion, nn.CrossEntropyLoss) and criterion.reduction == "mean" and criterion.weight is None
            and criterion.ignore_index == -100):
        if criterion.label_smoothing == 0.0:
            return train_ops.fused_cross_entropy
        return functools.partial(train_ops.fused_cross_entropy, label_smoothing=float(criterion.label_smoothing))
    return criterion


def _mixed_loss(loss_fn, output, label, label_b, lam):
    """The loss of a mixed batch: the HIP loss takes both labels; a foreign criterion is weighed as mixup defines it
    (``lam`` holds one value per batch, repeated per row)."""
    from sir_amd import slots, train_ops
    if getattr(loss_fn, "func", loss_fn) is train_ops.fused_cross_entropy or isinstance(loss_fn, slots.SlotLoss):
        return loss_fn(output, label, label_b, lam)
    return lam[0] * loss_fn(output, label) + (1.0 - lam[0]) * loss_fn(output, label_b)


def _step_loss(model, mel, label, loss_fn, mixup, adversary, metric):
    """The loss of one training step, for both epoch functions: mixup, then the adversary against the step's own loss (it returns
    a new tensor: ``mel`` itself -- the prefetcher's buffer -- is read, never written), then the loss of a mixed batch, or
    ``metric``'s (`metric_loss`: never together with mixup or an adversary, train() refuses that), or the plain one."""
    if mixup is not None:
        mel, label_b, lam = mixup(mel, label)

        def loss_of(out):
            return _mixed_loss(loss_fn, out, label, label_b, lam)
    else:
        def loss_of(out):
            return loss_fn(out, label)
    if adversary is not None:
        mel = adversary(model, mel, loss_of)
    if metric is not None and mixup is None:
        return metric.loss(model, mel, label, loss_fn)
    return loss_of(model(mel))


def loader_kwargs(num_workers):
    """How this package builds its DataLoaders (the ``hbm_feature_cache: false`` route of ``train()``, ``evaluate()``):
    * ``pin_memory=False`` -- host batches go through ``HostStager``'s persistent pinned ring instead of torch's per-batch pinning;
    * worker processes from a FORK SERVER, kept alive across epochs.  The reference's ``DataLoader(num_workers=8)`` forks its
      workers from the training process (train.py:203-219); on this stack, children forked from a process that has initialised
      HIP slow that process's GPU submissions ~50x for as long as they live (a 2 ms training step takes 70-100 ms: 3 k
      utterances/s; the same loader with fork-server workers: 34 k -- profiles/r04/dataloader_probe.txt).  Fork-server workers
      start from a clean process; the dataset travels to them by pickle once (``persistent_workers``)."""
    kw = dict(num_workers=num_workers, pin_memory=False)
    if num_workers > 0:
        kw.update(multiprocessing_context="forkserver", persistent_workers=True)
    return kw


def train_epoch(model, train_loader, optimizer, criterion, device, scaler=None, mixup=None):
    """One epoch (train.py:72-118); returns the mean of the per-step losses.  ``scaler`` is accepted
    for signature compatibility: the HIP path always computes in fp32 (the parity target is the fp32
    CPU path), so no loss scaling is needed or applied.  ``mixup`` (a ``train_ops.Mixup``): every assembled batch is
    mixed with a permutation of itself on the GPU and the loss takes both label sets.  An LR scheduler rides on the
    optimizer (``step_scheduler_with``): it is stepped after every ``optimizer.step()`` below, the zero-contribution step of
    an empty shard included, so every rank keeps the same learning rate.  A ``train_ops.Adversary`` rides on the model the same
    way (``train_ops.set_adversary(model, adversary)``: the signature stays the reference's): after mixup, the assembled batch is
    replaced by its adversarial example against the step's own loss (label smoothing and both mixup label sets included);
    crafting leaves the module untouched and holds no collective, so an empty-shard rank simply skips it."""
    from sir_amd import ops, train_ops
    adversary = train_ops.adversary_of(model)
    metric = train_ops.metric_loss_of(model)            # (`metric_loss`: never together with mixup or an adversary, train() refuses that)
    model.train()
    loss_fn = _loss_fn(criterion)
    losses = []
    stage = HostStager(device)
    pbar = tqdm(train_loader, desc="Training", disable=_quiet())
    for batch_idx, (mel, label) in enumerate(pbar):
        if mel is None or label is None or mel.size(0) == 0:
            if train_ops.world_size() > 1:
                # the other ranks are entering this step's gradient all-reduce: join it with a zero gradient and apply
                # the same update (a bare `continue`, train.py:82-83, would leave them waiting for ever)
                optimizer.zero_grad(set_to_none=True)
                train_ops.zero_contribution_step(model)
                if metric is not None:
                    metric.zero_contribution()
                optimizer.step()
            continue
        mel = stage(mel)                                   # host batches: persistent pinned ring (see HostStager)
        label = stage(label)
        optimizer.zero_grad(set_to_none=True)
        loss = _step_loss(model, mel, label, loss_fn, mixup, adversary, metric)
        loss.backward()
        if metric is not None:
            metric.sync_grad()
        optimizer.step()
        losses.append(loss.detach())
        if batch_idx % 10 == 0 and not _quiet():
            pbar.set_postfix({"loss": f"{loss.item():.4f}",
                              "GPU": f"{torch.cuda.memory_allocated() / 1024 ** 2:.1f}MB"})
    mean = torch.stack(losses).mean().item() if losses else 0.0      # one device->host sync per epoch
    ops.check_status()            # ... which is where a timed-out GRU recurrence is reported (on every rank: collective)
    return mean


def train_epoch_waveforms(model, wave_loader, optimizer, criterion, device, t_pad=200, augment=None, frontend=None, mixup=None):
    """``train_epoch`` fed with RAW waveform batches: ``wave_loader`` yields ``(wave [B, L] float32 | int16, lengths int32
    [B] | None, label int64 [B])``; the log-mel features are computed on the GPU (BASELINE configs[2]: fused HIP feature
    extraction + forward/backward + Adam) one batch ahead of the training step on a side stream
    (``sir_amd.pipeline.FeaturePrefetcher``).  Items may carry a fourth element, the lengths as a host list (what
    ``WaveformStore.epoch_batches`` yields), so that augmentation parameters can be drawn without a device sync.
    ``augment(wave_batch_index, batch_size, host_lengths | None) -> dict`` may return the featurizer's on-the-fly
    augmentation arguments (``shift``, ``noise_sigma``, ``noise_seed``, ``time_mask``, ``freq_mask``: scripts/augment.py,
    dataset.py:160-176) for that batch, ``pitch_cents`` / ``tempo`` (``sir_wave_perturb`` ahead of the feature kernel) and the
    reverb / background-noise arguments of ``HipFeaturizer.reverb_mix`` (between the two).
    ``mixup`` as for ``train_epoch``: applied to the computed feature batch, after its SpecAugment bands.
    An adversary set on the model (``train_ops.set_adversary``) as for ``train_epoch``: applied to the feature batch after mixup
    (the attack is on the features, not the audio).
    ``frontend`` (sir_amd/frontend_config.py; None = 1024 / 512 / 1024): the front-end the features are computed with.
    Returns the mean of the per-step losses."""
    from sir_amd import ops, train_ops
    from sir_amd.pipeline import FeaturePrefetcher
    adversary = train_ops.adversary_of(model)
    metric = train_ops.metric_loss_of(model)
    model.train()
    loss_fn = _loss_fn(criterion)
    pre = FeaturePrefetcher(t_pad=t_pad, frontend=frontend)
    losses, pending = [], []

    def submit(idx, item):
        wave, lengths, label = item[:3]
        host_lengths = item[3] if len(item) > 3 else None
        if wave is None or label is None or wave.size(0) == 0:
            return
        wave = wave.to(device, non_blocking=True)
        lengths = lengths.to(device, non_blocking=True) if lengths is not None else None
        pre.kw = augment(idx, wave.size(0), host_lengths) if augment is not None else {}
        pre.submit(wave, lengths)
        pending.append(label.to(device, non_blocking=True))

    def step():
        mel, label = pre.get(), pending.pop(0)
        optimizer.zero_grad(set_to_none=True)
        loss = _step_loss(model, mel, label, loss_fn, mixup, adversary, metric)
        loss.backward()
        if metric is not None:
            metric.sync_grad()
        optimizer.step()
        pre.release()
        losses.append(loss.detach())

    for idx, item in enumerate(tqdm(wave_loader, desc="Training", disable=_quiet())):
        submit(idx, item)
        if len(pending) == 2:                           # batch idx is queued: train on batch idx - 1 beside it
            step()
    while pending:
        step()
    mean = torch.stack(losses).mean().item() if losses else 0.0
    ops.check_status()
    return mean


def make_waveform_augment(config, seed=0, epoch=0, rng=None):
    """The ``augment`` callable of ``train_epoch_waveforms`` for the YAML keys of scripts/train.py: time shift + noise
    (scripts/augment.py:98-135 gating, ``waveform_augment_prob``, default 0.7 as augment.py:98) when
    ``waveform_augment`` is on, and the dataset's SpecAugment (dataset.py:105-106, :160-176, ``augment_prob``) always --
    the cached-feature route applies that one in ``FSCIntentDataset.__getitem__``, the fused route has no dataset.
    ``pitch_speed_augment`` (implies ``waveform_augment``) draws all four waveform effects of augment.py:119-133 --
    shift, pitch, speed, noise -- and adds ``pitch_cents`` / ``tempo``; the time masks are then drawn against the frame
    counts of the PERTURBED clips (known on the host from the tempo, no device sync).
    ``reverb_augment`` (``reverb_prob``, default 0.5; RIRs from the WAV files below ``rir_dir``, else 32 synthetic ones with
    RT60 drawn from ``rt60_range``, default 0.2-0.8 s) and ``background_noise_augment`` (``noise_prob``, default 0.5; clips
    from ``noise_dir``, else 8 synthetic coloured-noise clips; ``snr_db_range``, default 5-20 dB) add the arguments of
    ``HipFeaturizer.reverb_mix``: ``rir`` / ``noise`` (the banks) and ``rir_index``, ``noise_index``, ``noise_offset``,
    ``snr_db``, drawn after every other draw of the batch.  Neither changes a clip's length.  With both keys absent or
    false the random stream and the returned dictionary are what they were without them."""
    import random
    from sir_amd.frontend_config import FrontEnd
    from sir_amd.scripts import augment as aug
    fe = FrontEnd.from_config(config)                   # the time masks are drawn against the clips' frame counts
    rng = rng or random.Random((int(seed) << 20) ^ int(epoch))
    banks = _reverb_noise_banks(config, seed)
    pitch_speed = bool(config.get("pitch_speed_augment", False))
    wave_aug = bool(config.get("waveform_augment", False)) or pitch_speed
    wave_prob = float(config.get("waveform_augment_prob", 0.7))
    spec_prob = float(config.get("augment_prob", 0.5))

    def fn(idx, bsz, host_lengths):
        if host_lengths is None:
            raise ValueError("waveform augmentation needs the clip lengths on the host (WaveformStore yields them)")
        kw = {}
        frame_lengths = host_lengths
        if pitch_speed:
            shift, cents, tempo, sigma = aug.draw_batch_params_full(host_lengths, wave_prob, rng)
            kw.update(shift=shift, pitch_cents=cents, tempo=tempo, noise_sigma=sigma,
                      noise_seed=(int(seed) << 40) ^ (int(epoch) << 24) ^ int(idx))
            frame_lengths = [aug.perturbed_out_len(n, f) for n, f in zip(host_lengths, tempo.tolist())]
        elif wave_aug:
            shift, sigma = aug.draw_batch_params(host_lengths, wave_prob, rng)
            kw.update(shift=shift, noise_sigma=sigma, noise_seed=(int(seed) << 40) ^ (int(epoch) << 24) ^ int(idx))
        if spec_prob > 0.0:
            tm, fm = aug.draw_spec_masks([fe.num_frames(n) for n in frame_lengths], spec_prob, rng=rng)
            kw.update(time_mask=tm, freq_mask=fm)
        if banks:
            kw.update(aug.draw_reverb_noise_params(frame_lengths, banks["cfg"], rng))
            if "rir_index" in kw:
                kw["rir"] = banks["rir"]
            if "noise_index" in kw:
                kw["noise"] = banks["noise"]
        return kw
    return fn


_bank_cache = {}


def _reverb_noise_banks(config, seed=0):
    """The ``SoundBank``s and draw settings of ``reverb_augment`` / ``background_noise_augment`` (None when both are off),
    built once per distinct setting and kept on the host until the first batch stages them on its device."""
    reverb = bool(config.get("reverb_augment", False))
    noise = bool(config.get("background_noise_augment", False))
    if not (reverb or noise):
        return None
    import numpy as np
    from sir_amd import synth
    from sir_amd.sound_bank import SoundBank
    rt60 = tuple(float(v) for v in config.get("rt60_range", (0.2, 0.8)))
    key = (reverb, config.get("rir_dir"), rt60, noise, config.get("noise_dir"), int(seed))
    if key not in _bank_cache:
        gen = np.random.default_rng([int(seed) & 0xFFFFFFFF, 0x52495253])      # its own stream: not the batch draws' rng
        rir = nb = None
        if reverb:
            if config.get("rir_dir"):
                rir = SoundBank.from_dir(config["rir_dir"], kind="rir")
            else:
                rir = SoundBank([synth.synthetic_rir(gen.uniform(*rt60), rng=gen) for _ in range(32)], kind="rir")
        if noise:
            if config.get("noise_dir"):
                nb = SoundBank.from_dir(config["noise_dir"], kind="noise", max_seconds=60.0)
            else:
                nb = SoundBank([synth.coloured_noise(10 * synth.SAMPLE_RATE, gen, exponent=e) for e in (0.0, 0.5, 1.0, 1.0, 1.5, 1.5, 2.0, 2.0)])
        _bank_cache[key] = (rir, nb)
    rir, nb = _bank_cache[key]
    cfg = {"snr_db_range": tuple(config.get("snr_db_range", (5.0, 20.0)))}
    if rir is not None:
        cfg.update(n_rir=len(rir), reverb_prob=float(config.get("reverb_prob", 0.5)))
    if nb is not None:
        cfg.update(noise_lengths=nb.host_lengths, noise_prob=float(config.get("noise_prob", 0.5)))
    return {"rir": rir, "noise": nb, "cfg": cfg}


def build_lr_scheduler(optimizer, spec):
    """The ``lr_schedule`` YAML key -> a ``torch.optim.lr_scheduler`` object on ``optimizer`` (``FusedAdam`` reads
    ``group["lr"]`` every step), stepped once per optimizer step; ``None`` for an absent / empty key.

    ``{warmup_steps: W, kind: constant | cosine | step, min_lr, total_steps, step_size, gamma}``:
    ``W > 0`` puts ``LinearLR(start_factor=1 / (W + 1), total_iters=W)`` in front (step k runs at ``lr * (k + 1) / (W + 1)``,
    the full rate from step W on) under ``SequentialLR``; behind it ``cosine`` is ``CosineAnnealingLR(T_max=total_steps - W,
    eta_min=min_lr)`` (``total_steps`` optimizer steps in all: ``train()`` fills it in from the epoch count), ``step`` is
    ``StepLR(step_size, gamma)``, ``constant`` is ``LambdaLR`` with factor 1."""
    from torch.optim import lr_scheduler as sched
    if not spec:
        return None
    unknown = set(spec) - {"warmup_steps", "kind", "min_lr", "total_steps", "step_size", "gamma"}
    if unknown:
        raise ValueError(f"lr_schedule: unknown keys {sorted(unknown)}")
    kind = spec.get("kind", "constant")
    warm = int(spec.get("warmup_steps", 0))
    if warm < 0:
        raise ValueError("lr_schedule: warmup_steps must be >= 0")
    if kind == "constant":
        main = sched.LambdaLR(optimizer, lambda step: 1.0)
    elif kind == "cosine":
        if "total_steps" not in spec:
            raise ValueError("lr_schedule: kind cosine needs total_steps")
        t_max = int(spec["total_steps"]) - warm
        if t_max < 1:
            raise ValueError(f"lr_schedule: total_steps {spec['total_steps']} must exceed warmup_steps {warm}")
        main = sched.CosineAnnealingLR(optimizer, T_max=t_max, eta_min=float(spec.get("min_lr", 0.0)))
    elif kind == "step":
        if "step_size" not in spec:
            raise ValueError("lr_schedule: kind step needs step_size")
        main = sched.StepLR(optimizer, step_size=int(spec["step_size"]), gamma=float(spec.get("gamma", 0.1)))
    else:
        raise ValueError(f"lr_schedule: kind {kind!r} is not one of constant, cosine, step")
    if warm == 0:
        return main
    warmup = sched.LinearLR(optimizer, start_factor=1.0 / (warm + 1), end_factor=1.0, total_iters=warm)
    return sched.SequentialLR(optimizer, [warmup, main], milestones=[warm])


def step_scheduler_with(optimizer, scheduler):
    """Step ``scheduler`` once after every ``optimizer.step()`` (a step post-hook of the optimizer: ``train_epoch`` and
    ``train_epoch_waveforms`` keep the reference's signatures, and no call site of ``optimizer.step()`` can forget it -- the
    zero-contribution step of an empty shard steps it too).  Returns the hook's handle (``.remove()`` detaches it)."""
    return optimizer.register_step_post_hook(lambda opt, args, kwargs: scheduler.step())


ADVERSARIAL_KEYS = ("eps", "alpha", "steps", "random_start", "prob", "validate")


def adversarial_options(config):
    """The ``adversarial`` YAML key of ``train()`` -- ``{eps, alpha, steps, random_start, prob, validate}``, absent by default --
    as the keyword arguments of ``train_ops.Adversary`` plus ``validate``; ``None`` when the key is absent or empty.  Raises
    ``ValueError`` for unknown keys, a missing or negative ``eps``, ``steps < 1``, ``prob`` outside [0, 1] or a negative
    ``alpha``: on the host, before any device call."""
    spec = config.get("adversarial")
    if not spec:
        return None
    if not isinstance(spec, dict):
        raise ValueError("adversarial: expected a mapping {eps, alpha, steps, random_start, prob, validate}")
    unknown = set(spec) - set(ADVERSARIAL_KEYS)
    if unknown:
        raise ValueError(f"adversarial: unknown keys {sorted(unknown)}")
    if "eps" not in spec:
        raise ValueError("adversarial: eps is required")
    eps, steps, prob = float(spec["eps"]), int(spec.get("steps", 1)), float(spec.get("prob", 1.0))
    alpha = float(spec["alpha"]) if spec.get("alpha") is not None else None
    if not eps >= 0.0:
        raise ValueError("adversarial: eps must be >= 0")
    if steps < 1:
        raise ValueError("adversarial: steps must be >= 1")
    if not 0.0 <= prob <= 1.0:
        raise ValueError("adversarial: prob must be in [0, 1]")
    if alpha is not None and not alpha >= 0.0:
        raise ValueError("adversarial: alpha must be >= 0")
    return {"eps": eps, "alpha": alpha, "steps": steps, "random_start": bool(spec.get("random_start", True)), "prob": prob,
            "validate": bool(spec.get("validate", False))}


def metric_loss_options(config):
    """The ``metric_loss`` YAML key of ``train()`` -- ``{weight, ce_weight, scale, margin, bank_out}``, absent by default -- on the
    host, before any device call: None, or the five values with their defaults (weight 1, ce_weight 1, scale 16, margin 0.1,
    bank_out None).  The step's loss becomes ``ce_weight * CE(logits) + weight * ProxyHead(emb, labels)`` (DESIGN.md section 4,
    "Training the embedding").  ``ValueError`` for unknown keys, a negative weight, ``scale <= 0``, ``margin < 0``, both weights
    zero, and for ``metric_loss`` together with ``mixup``, ``adversarial`` or ``slots``: a proxy loss needs one hard label per
    clip and its own crafting loss, which is out of scope."""
    spec = config.get("metric_loss")
    if spec is None or spec is False:
        return None
    if not isinstance(spec, dict):
        raise ValueError("metric_loss: expected a mapping {weight, ce_weight, scale, margin, bank_out}")
    unknown = set(spec) - {"weight", "ce_weight", "scale", "margin", "bank_out"}
    if unknown:
        raise ValueError(f"metric_loss: unknown keys {sorted(unknown)}")
    for other in ("mixup", "adversarial", "slots"):
        if config.get(other):
            raise ValueError(f"metric_loss cannot be combined with {other}: the proxy loss takes one hard label per clip")
    out = {"weight": float(spec.get("weight", 1.0)), "ce_weight": float(spec.get("ce_weight", 1.0)),
           "scale": float(spec.get("scale", 16.0)), "margin": float(spec.get("margin", 0.1)), "bank_out": spec.get("bank_out")}
    if not out["weight"] >= 0.0 or not out["ce_weight"] >= 0.0:
        raise ValueError("metric_loss: weight and ce_weight must be >= 0")
    if out["weight"] == 0.0 and out["ce_weight"] == 0.0:
        raise ValueError("metric_loss: weight and ce_weight are both zero: nothing would be trained")
    if not (out["scale"] > 0.0 and out["scale"] < float("inf")):
        raise ValueError("metric_loss: scale must be positive and finite")
    if not (out["margin"] >= 0.0 and out["margin"] < float("inf")):
        raise ValueError("metric_loss: margin must be finite and >= 0")
    if out["bank_out"] is not None and (not isinstance(out["bank_out"], str) or not out["bank_out"]):
        raise ValueError("metric_loss: bank_out is a file name")
    return out


def validate_robust(model, val_loader, device, eps, **pgd_kw):
    """Robust validation accuracy: the share of the loader's clips still classified correctly after ``explain.pgd`` (eval
    semantics; all-zero padding columns kept) at radius ``eps``; under data parallelism the counts are summed over ranks."""
    from sir_amd import explain, ops, train_ops
    model.eval()
    stage = HostStager(device)
    counts = torch.zeros(3, dtype=torch.int64, device=device)         # clean correct, adversarial correct, clips
    for mel, label in val_loader:
        if mel is None or label is None or mel.size(0) == 0:
            continue
        mel, label = stage(mel), stage(label)
        clean, adv = explain.robust_accuracy(model, mel, label, eps, keep_zero_columns=True, **pgd_kw)
        counts += torch.stack([clean, adv, torch.full_like(clean, label.size(0))])
    ops.check_status()
    train_ops.all_reduce_sum_(counts)
    clean, adv, total = (int(v) for v in counts.tolist())
    return clean / max(total, 1), adv / max(total, 1)


def run_options(config):
    """The run-management YAML keys of ``train()`` as one dict, every one absent by default (= no scheduler, no shadow, no
    ``latest_checkpoint.pt``, plain Adam): ``optimizer: adam | adamw``, ``lr_schedule``, ``ema_decay`` / ``ema_warmup``,
    ``checkpoint_every_epoch``, ``resume: <path> | true`` (``true`` = ``save_path/latest_checkpoint.pt``)."""
    from sir_amd import run_state
    kind = str(config.get("optimizer", "adam")).lower()
    if kind not in ("adam", "adamw"):
        raise ValueError(f"optimizer: {kind!r} is not one of adam, adamw")
    ema = config.get("ema_decay")
    if not ema and config.get("ema_warmup"):
        raise ValueError("ema_warmup needs ema_decay")
    latest = os.path.join(config.get("save_path", "checkpoints/"), run_state.LATEST)
    resume = config.get("resume")
    return {"decoupled_weight_decay": kind == "adamw",
            "ema_decay": float(ema) if ema else None,
            "ema_warmup": bool(config.get("ema_warmup", False)),
            "lr_schedule": dict(config["lr_schedule"]) if config.get("lr_schedule") else None,
            "checkpoint_path": latest if config.get("checkpoint_every_epoch") else None,
            "resume_path": None if not resume else (latest if resume is True else str(resume))}


def slot_options(config, train_csv=None):
    """The YAML key ``slots: {columns, map, weights}`` (absent by default) -> None or ``{"spec", "weights"}``, on the host.
    ``map``: a ``slot_map.json`` written by ``SlotSpec.save`` (absent: the vocabularies are built from the training CSV's
    ``columns``, default action / object / location); ``weights``: one loss weight per slot.  ``num_labels`` must be the sum
    of the slot widths: the model's ``fc`` writes exactly those logits."""
    opts = config.get("slots")
    if not opts:
        return None
    from sir_amd import slots
    if not isinstance(opts, dict):
        raise ValueError("`slots` must be a mapping with the keys columns / map / weights")
    unknown = sorted(set(opts) - {"columns", "map", "weights"})
    if unknown:
        raise ValueError(f"`slots` has unknown keys {unknown}")
    columns = tuple(opts.get("columns") or ("action", "object", "location"))
    if opts.get("map"):
        spec = slots.SlotSpec.load(opts["map"])
        if opts.get("columns") and tuple(spec.columns) != columns:
            raise ValueError(f"`slots.columns` {list(columns)} differ from those of {opts['map']}: {list(spec.columns)}")
    else:
        spec = slots.SlotSpec.from_csv(train_csv, columns)
    num_labels = config.get("num_labels", 31)
    if num_labels != spec.total:
        raise ValueError(f"num_labels is {num_labels}, the slot layout {dict(zip(spec.columns, spec.sizes))} needs {spec.total}")
    return {"spec": spec, "weights": slots.check_weights(opts.get("weights"), spec.n_slots)}


def validate(model, val_loader, criterion, device, scaler=None):
    """(avg_loss, accuracy) over the loader (train.py:120-155); under data parallelism the counts are
    summed over ranks.  With 2-D labels (slot heads) the accuracy is the exact-match rate over the slots."""
    from sir_amd import ops, train_ops
    model.eval()
    loss_fn = _loss_fn(criterion)
    losses = []
    correct = torch.zeros((), dtype=torch.int64, device=device)
    total = 0
    stage = HostStager(device)
    with torch.no_grad():
        for mel, label in tqdm(val_loader, desc="Validating", disable=_quiet()):
            if mel is None or label is None or mel.size(0) == 0:
                continue
            mel = stage(mel)
            label = stage(label)
            output, predicted = model.predict(mel)
            losses.append(loss_fn(output, label))
            if label.dim() == 2:
                # slot heads (the criterion is a slots.SlotLoss): a clip is right when every slot is (exact match); the argmax
                # over the whole row means nothing here
                from sir_amd import slots
                idx, _, _ = slots.classify(output, criterion.spec, k=1)
                correct += (idx[:, :, 0] == label).all(dim=1).sum()
            else:
                correct += (predicted == label).sum()
            total += label.size(0)
    counts = torch.tensor([int(correct.item()), total], dtype=torch.int64, device=device)
    ops.check_status()                                # the host has just synchronised: surface a timed-out recurrence
    train_ops.all_reduce_sum_(counts)
    accuracy = counts[0].item() / max(counts[1].item(), 1)
    avg_loss = torch.stack(losses).mean().item() if losses else 0.0
    return avg_loss, accuracy


def _quiet():
    return int(os.environ.get("RANK", "0")) != 0


def train(args, config):
    """Main training function (train.py:164-302): same YAML keys, same best-checkpoint rule
    (bare ``state_dict`` at ``save_path/best_model.pt``), same early stopping.

    Run management (``run_options``, all keys absent by default): with ``checkpoint_every_epoch`` the whole run state
    (``sir_amd.run_state``) goes to ``save_path/latest_checkpoint.pt`` after each epoch's validation, and ``resume`` picks a
    run up at that epoch boundary.  On the ``hbm_feature_cache`` (default) and ``fused_features`` / ``waveform_augment``
    routes the resumed run is bit-identical to the uninterrupted one: data order and augmentation there are pure functions
    of ``(seed, epoch, rank)``.  The DataLoader route (``hbm_feature_cache: false``) draws SpecAugment from its worker
    processes' global RNGs: it resumes, but not bit-exactly.  A run cut off inside an epoch repeats that epoch."""
    from sir_amd import _native, run_state, train_ops  # noqa: F401
    from sir_amd.frontend_config import FrontEnd
    from sir_amd.models.models import CNNAudioGRU
    from sir_amd.optim import FusedAdam
    from sir_amd.scripts.dataset import FSCIntentDataset

    adv_opts = adversarial_options(config)            # (a bad `adversarial` key raises here, before any device call)
    metric_opts = metric_loss_options(config)         # (and a bad `metric_loss` key, or one beside mixup / adversarial / slots)
    # `slots: {columns, map, weights}` (absent by default): slot heads -- the label of a clip is one class per CSV column, the
    # loss a weighted sum of per-segment cross-entropies, the validation accuracy the exact-match rate (sir_amd/slots.py,
    # DESIGN.md section 4).  A layout that does not add up to `num_labels` raises here, before any device call.
    slot_opts = slot_options(config, args.train_csv)
    slot_spec = slot_opts["spec"] if slot_opts else None
    _native.require_hip()
    train_ops.limit_host_threads(reserve=int(config.get("num_workers", 2)))     # (the DataLoader workers get their share of the CPU quota)
    rank, world, local_rank = train_ops.init_distributed()
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    if rank == 0:
        print(f"Training on: {device} ({torch.cuda.get_device_name(local_rank)}), world size {world}")

    cache_dir = config.get("cache_dir", "data/cached_features")
    use_cache = config.get("use_feature_cache", True)
    # `n_fft` / `hop_length` / `win_length` (defaults 1024 / 512 / n_fft): the feature front-end, read once and handed to every
    # route below; `mel_spec_length` is the model's t_pad (3 s at hop 160 is 301 frames).
    fe = FrontEnd.from_config(config)
    fe_kw = dict(n_fft=fe.n_fft, hop_length=fe.hop_length, win_length=fe.win_length)
    # Two YAML keys beyond the reference's, both off by default (= reference behaviour: cached features through
    # DataLoader workers).  `fused_features: true` trains from RAW waveforms staged once in HBM, features computed on
    # the GPU inside the step (BASELINE configs[2]); `waveform_augment: true` (implies fused_features) adds the
    # time-shift / noise augmentation of scripts/augment.py inside the feature kernel (configs[4]).
    # `hbm_feature_cache` (default true): the cached-feature route keeps the split's cache in HBM (sir_amd/feature_store.py) and
    # assembles each batch with one gather launch instead of DataLoader workers + a host -> device copy per step -- same files,
    # same item semantics; false = the reference's DataLoader route, which at batch 256 delivers a fraction of what the training
    # step consumes (bench.py `dropin_epoch`).
    # `pitch_speed_augment: true` (implies waveform_augment) adds the pitch and speed effects of scripts/augment.py on the GPU
    # (sir_wave_perturb ahead of the feature kernel).
    # `reverb_augment: true` / `background_noise_augment: true` (each implies fused_features, not waveform_augment) add room
    # reverberation and background noise at a drawn SNR (sir_wave_reverb_mix between the two).
    wave_aug = bool(config.get("waveform_augment", False)) or bool(config.get("pitch_speed_augment", False))
    fused = bool(config.get("fused_features", False)) or wave_aug or bool(config.get("reverb_augment", False)) \
        or bool(config.get("background_noise_augment", False))
    hbm_cache = bool(config.get("hbm_feature_cache", True)) and not fused
    train_store = None
    if fused:
        from sir_amd.waveform_store import WaveformStore
        train_store = WaveformStore(args.train_csv, args.label_map, device,
                                    sample_rate=int(config.get("sample_rate", 16000)), slot_spec=slot_spec)
    t_pad = int(config.get("mel_spec_length", MAX_LENGTH))
    if hbm_cache:
        from sir_amd.feature_store import FeatureStore
        train_dataset = FeatureStore(args.train_csv, args.label_map, device, use_cache=use_cache, cache_dir=cache_dir, mel_spec_length=t_pad,
                                     frontend=fe, slot_spec=slot_spec)
        val_dataset = FeatureStore(args.val_csv, args.label_map, device, use_cache=use_cache, cache_dir=cache_dir, mel_spec_length=t_pad,
                                   frontend=fe, slot_spec=slot_spec)
    else:
        train_dataset = train_store if fused else \
            FSCIntentDataset(csv_path=args.train_csv, label_map_path=args.label_map, is_training=True,
                             augment_prob=config.get("augment_prob", 0.5), use_cache=use_cache, cache_dir=cache_dir,
                             mel_spec_length=t_pad, slot_spec=slot_spec, **fe_kw)
        val_dataset = FSCIntentDataset(csv_path=args.val_csv, label_map_path=args.label_map, is_training=False,
                                       use_cache=use_cache, cache_dir=cache_dir, mel_spec_length=t_pad, slot_spec=slot_spec, **fe_kw)
    if rank == 0:
        print(f"Datasets loaded - Train: {len(train_dataset)}, Val: {len(val_dataset)}")

    bs = config["batch_size"]                      # per-GPU batch; the global batch is bs * world
    nw = config.get("num_workers", 2)
    seed = int(config.get("seed", 0))
    train_sampler = train_ops.ShardSampler(len(train_dataset), rank, world, shuffle=True, seed=seed)
    val_sampler = train_ops.ShardSampler(len(val_dataset), rank, world, shuffle=False, pad=False)
    lkw = loader_kwargs(nw)
    train_loader = None if (fused or hbm_cache) else DataLoader(train_dataset, batch_size=bs, sampler=train_sampler, collate_fn=collate_fn, **lkw)
    val_loader = None if hbm_cache else DataLoader(val_dataset, batch_size=bs * 2, sampler=val_sampler, collate_fn=collate_fn, **lkw)

    model = CNNAudioGRU(num_classes=config.get("num_labels", 31)).to(device)
    # Two more YAML keys, both absent by default (= the reference: train everything from scratch).  `init_checkpoint`: a
    # state dict or {'model_state_dict': ...} file whose body is kept and whose `fc` is re-initialised when its label set
    # differs from `num_labels`; `freeze`: a list out of bn_stats / cnn / gru / attention (sir_amd/finetune.py).
    if config.get("init_checkpoint"):
        from sir_amd import finetune
        report = finetune.load_pretrained(model, config["init_checkpoint"])
        if rank == 0:
            print(f"init_checkpoint: kept {len(report['kept'])} tensors, re-initialised {report['reset'] or 'nothing'}")
    if config.get("freeze"):
        from sir_amd import finetune
        what = [config["freeze"]] if isinstance(config["freeze"], str) else list(config["freeze"])      # (a YAML scalar or a list)
        trainable = finetune.freeze(model, what)
        if rank == 0:
            print(f"freeze {sorted(what)}: {len(trainable)} trainable tensors")
    train_ops.broadcast_module_(model)             # identical initial weights / BN buffers on every rank
    # Three more YAML keys, all absent by default (= the reference's step: hard labels, unclipped gradients).
    # `label_smoothing: <eps>` and `mixup: <alpha>` change the training loss (validation keeps the plain criterion);
    # `clip_grad_norm: <max_norm>` clips the global gradient norm inside the optimizer step.  The reference's own
    # `grad_clip` / `mixup_alpha` keys stay unread, as the reference leaves them.
    # `adversarial: {eps, alpha, steps, random_start, prob, validate}` (absent by default): FGSM / PGD adversarial training in
    # the feature domain -- each assembled batch is replaced by its adversarial example against the step's own loss
    # (train_ops.Adversary); `validate: true` also logs the robust validation accuracy per epoch.
    opts = run_options(config)
    criterion = nn.CrossEntropyLoss()
    train_criterion = nn.CrossEntropyLoss(label_smoothing=float(config["label_smoothing"])) if config.get("label_smoothing") else criterion
    if slot_opts:                                     # label smoothing folded in; validation keeps the plain (weighted) slot loss
        from sir_amd import slots
        criterion = slots.SlotLoss(slot_spec, slot_opts["weights"])
        train_criterion = slots.SlotLoss(slot_spec, slot_opts["weights"], float(config.get("label_smoothing") or 0.0))
    mixup = train_ops.Mixup(float(config["mixup"]), seed=seed + 977 * rank) if config.get("mixup") else None
    adversary = None
    if adv_opts:
        adversary = train_ops.Adversary(adv_opts["eps"], alpha=adv_opts["alpha"], steps=adv_opts["steps"],
                                        random_start=adv_opts["random_start"], prob=adv_opts["prob"], seed=seed + 1231 * rank)
    train_ops.set_adversary(model, adversary)         # rides on the model: train_epoch / train_epoch_waveforms keep their signatures
    # `metric_loss: {weight, ce_weight, scale, margin, bank_out}` (absent by default): a cosine-proxy loss on the embedding beside
    # the cross-entropy (prototypes.ProxyHead, DESIGN.md section 4 "Training the embedding").  The proxies are a second parameter
    # group; their state goes to `proxy_head.pt` beside every checkpoint and, as a PrototypeBank, to `bank_out` at the end.
    metric = None
    if metric_opts:
        from sir_amd.prototypes import ProxyHead
        head = ProxyHead(int(config.get("num_labels", 31)), scale=metric_opts["scale"], margin=metric_opts["margin"], seed=seed).to(device)
        if opts["resume_path"]:
            run_state.load_proxy_head(os.path.dirname(os.path.abspath(opts["resume_path"])), head)
        train_ops.broadcast_module_(head)
        metric = train_ops.MetricLoss(head, metric_opts["weight"], metric_opts["ce_weight"])
    train_ops.set_metric_loss(model, metric)
    trainable = [p for p in model.parameters() if p.requires_grad]
    optimizer = FusedAdam(trainable if metric is None else [{"params": trainable}, {"params": [metric.head.proxies]}],
                          lr=float(config.get("lr", 0.0003)),
                          weight_decay=float(config.get("weight_decay", 0.0001)),
                          max_grad_norm=float(config["clip_grad_norm"]) if config.get("clip_grad_norm") else None,
                          decoupled_weight_decay=opts["decoupled_weight_decay"], ema_decay=opts["ema_decay"],
                          ema_warmup=opts["ema_warmup"])
    if config.get("use_amp", True) and rank == 0:
        print("use_amp requested: the HIP path computes in fp32 (parity with the fp32 CPU path); no GradScaler")

    epochs = config.get("epochs", 20)
    patience = config.get("early_stop_patience", 5)
    best_val_acc = 0
    no_improve_count = 0
    scheduler = None
    if opts["lr_schedule"]:
        spec = opts["lr_schedule"]
        if spec.get("kind") == "cosine" and "total_steps" not in spec:      # the whole run: every rank takes the same step count
            n_shard = len(train_ops.ShardSampler(len(train_dataset), rank, world))
            spec["total_steps"] = epochs * ((n_shard + bs - 1) // bs)
        scheduler = build_lr_scheduler(optimizer, spec)
        step_scheduler_with(optimizer, scheduler)
    first_epoch = 0
    if opts["resume_path"]:
        got = run_state.load_run_state(opts["resume_path"], model, optimizer, scheduler, mixup, config=config, adversary=adversary)
        first_epoch, best_val_acc, no_improve_count = got["epoch"] + 1, got["best_val_acc"], got["no_improve_count"]
        if rank == 0:
            print(f"Resumed {opts['resume_path']}: epoch {first_epoch} done, best accuracy {best_val_acc:.4f}"
                  + (f"; config keys that differ from the saved run: {got['config_changed']}" if got["config_changed"] else ""))
    for epoch in range(first_epoch, epochs):
        if no_improve_count >= patience:              # (a resumed run that had already stopped early)
            break
        if rank == 0:
            print(f"\nEpoch {epoch + 1}/{epochs}")
        if fused:
            batches = train_store.epoch_batches(bs, rank, world, shuffle=True, seed=seed, epoch=epoch)
            train_loss = train_epoch_waveforms(model, batches, optimizer, train_criterion, device,
                                               t_pad=t_pad,
                                               augment=make_waveform_augment(config, seed=seed + 977 * rank, epoch=epoch),
                                               mixup=mixup, frontend=fe)
        elif hbm_cache:
            batches = train_dataset.epoch_batches(bs, rank, world, shuffle=True, seed=seed, epoch=epoch,
                                                  augment_prob=float(config.get("augment_prob", 0.5)))
            train_loss = train_epoch(model, batches, optimizer, train_criterion, device, None, mixup=mixup)
        else:
            train_sampler.set_epoch(epoch)
            train_loss = train_epoch(model, train_loader, optimizer, train_criterion, device, None, mixup=mixup)
        if hbm_cache:
            val_loader = val_dataset.epoch_batches(bs * 2, rank, world, shuffle=False, pad=False)
        if opts["ema_decay"] is not None:             # validate (and keep as best model) the averaged weights
            with optimizer.swapped_ema():
                val_loss, val_acc = validate(model, val_loader, criterion, device, None)
        else:
            val_loss, val_acc = validate(model, val_loader, criterion, device, None)
        if rank == 0:
            print(f"Train loss: {train_loss:.4f}, Val loss: {val_loss:.4f}, Val accuracy: {val_acc:.4f}")
        if adv_opts and adv_opts["validate"]:         # the same attack as in training, from the clip itself, eval semantics
            if hbm_cache:
                val_loader = val_dataset.epoch_batches(bs * 2, rank, world, shuffle=False, pad=False)
            _, robust_acc = validate_robust(model, val_loader, device, adv_opts["eps"], alpha=adv_opts["alpha"],
                                            steps=adv_opts["steps"])
            if rank == 0:
                print(f"Robust val accuracy (eps {adv_opts['eps']:g}, {adv_opts['steps']} steps): {robust_acc:.4f}")
        if val_acc > best_val_acc:
            best_val_acc = val_acc
            no_improve_count = 0
            if rank == 0:
                save_path = config.get("save_path", "checkpoints/")
                os.makedirs(save_path, exist_ok=True)
                best_sd = optimizer.ema_state_dict(model) if opts["ema_decay"] is not None else model.state_dict()
                torch.save(best_sd, os.path.join(save_path, "best_model.pt"))
                print(f"New best model saved with accuracy: {val_acc:.4f}")
        else:
            no_improve_count += 1
            if rank == 0:
                print(f"No improvement for {no_improve_count} epochs")
        if opts["checkpoint_path"]:                   # after the bookkeeping above: a resumed run starts at epoch + 1
            run_state.save_run_state(opts["checkpoint_path"], model, optimizer, scheduler, mixup, epoch=epoch,
                                     best_val_acc=best_val_acc, no_improve_count=no_improve_count, config=config,
                                     adversary=adversary)
            if metric is not None and rank == 0:
                run_state.save_proxy_head(os.path.dirname(os.path.abspath(opts["checkpoint_path"])), metric.head)
        if no_improve_count >= patience:
            if rank == 0:
                print(f"Early stopping after {epoch + 1} epochs")
            break
    if metric is not None and rank == 0:
        from sir_amd.prototypes import PrototypeBank
        save_path = config.get("save_path", "checkpoints/")
        os.makedirs(save_path, exist_ok=True)
        run_state.save_proxy_head(save_path, metric.head)
        if metric_opts["bank_out"]:
            bank_out = metric_opts["bank_out"]
            PrototypeBank.from_proxies(metric.head).save(bank_out if os.path.isabs(bank_out) else os.path.join(save_path, bank_out))
    if rank == 0:
        print(f"Training completed. Best validation accuracy: {best_val_acc:.4f}")
    train_ops.shutdown_distributed()
    return best_val_acc


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description="Train intent recognition model")
    parser.add_argument("--config", type=str, default="configs/config.yaml", help="Path to config file")
    parser.add_argument("--train_csv", type=str, default=None, help="Path to training CSV")
    parser.add_argument("--val_csv", type=str, default=None, help="Path to validation CSV")
    parser.add_argument("--label_map", type=str, default="data/processed/label_map.json",
                        help="Path to label map JSON file")
    args = parser.parse_args()
    config = load_config(args.config)
    if args.train_csv is None:
        args.train_csv = config.get("train_csv")
    if args.val_csv is None:
        args.val_csv = config.get("valid_csv")
    train(args, config)
