"""The state of a training RUN, saved and loaded so that the run continues bit for bit at an epoch boundary.

What a run carries from one epoch into the next is defined by what the step reads:

* the model's parameters and BatchNorm buffers;
* the optimizer's step count, both moments and (with ``ema_decay``) the shadow -- ``FusedAdam.state_dict()``, keyed by
  group index -- plus the learning rate the scheduler left in ``param_groups``;
* the LR scheduler's own counters;
* the dropout step counter of ``train_ops`` (the key of every inter-layer dropout mask), per rank;
* ``Mixup.rng`` and ``Adversary.rng`` (one host ``random.Random`` each per rank);
* the epoch number, ``best_val_acc`` and the early-stopping count.

Data order and augmentation are NOT part of it on the two routes that guarantee a bit-exact resume: there they are pure
functions of ``(seed, epoch, rank)`` (``FeatureStore.epoch_batches``, ``WaveformStore.epoch_batches``,
``scripts.train.make_waveform_augment`` all build their generators from those three numbers per epoch).  The DataLoader
route (``hbm_feature_cache: false``) draws SpecAugment from the worker processes' global RNGs, which nothing here
captures: it resumes, but not bit-exactly.  Resume granularity is the epoch boundary; a run cut off inside an epoch
repeats that epoch from the last file.

The file is a ``torch.save`` dict.  The model sits under ``model_state_dict``, the key under which the reference's
checkpoint loaders (and ``scripts/evaluate.py`` / ``finetune.load_pretrained`` here) look for it.  Rank 0 writes it to a temporary
file beside the target and renames it over the target (``os.replace``): a reader finds the previous file or the new one,
never a partial one.  The per-rank items travel to rank 0 with ``all_gather_object``; every rank reads the file and takes
its own entry.
"""
import os

import torch

from . import dist_utils, train_ops

FORMAT = 1
LATEST = "latest_checkpoint.pt"
# the YAML keys of scripts/train.py that shape the saved state (kept in the file; `load_run_state` reports the ones that
# differ from the resuming run's)
STATE_KEYS = ("optimizer", "lr", "weight_decay", "clip_grad_norm", "lr_schedule", "ema_decay", "ema_warmup", "mixup",
              "label_smoothing", "batch_size", "seed", "num_labels", "freeze", "adversarial")


def _rank_world(rank, world):
    if world is None:
        world = dist_utils.world_size()
    if rank is None:
        rank = torch.distributed.get_rank() if world > 1 else 0
    return int(rank), int(world)


def param_layout(optimizer):
    """Element counts of the tensors of every parameter group: what the flat optimizer buffers are laid out by."""
    return [[int(p.numel()) for p in group["params"]] for group in optimizer.param_groups]


def state_config(config):
    return {k: config[k] for k in STATE_KEYS if k in (config or {})}


def save_run_state(path, model, optimizer, scheduler=None, mixup=None, epoch=0, best_val_acc=0.0, no_improve_count=0,
                   config=None, rank=None, world=None, adversary=None):
    """Write the run state AFTER epoch ``epoch`` (0-based: the resumed run starts at ``epoch + 1``).  Collective when
    ``world > 1``: every rank calls it; rank 0 writes.  Returns ``path`` on rank 0, ``None`` elsewhere."""
    rank, world = _rank_world(rank, world)
    mine = {"dropout_step": train_ops.dropout_step(), "mixup_rng": mixup.rng.getstate() if mixup is not None else None,
            "adversary_rng": adversary.rng.getstate() if adversary is not None else None}
    per_rank = [mine]
    if world > 1 and torch.distributed.is_available() and torch.distributed.is_initialized():
        per_rank = [None] * world
        torch.distributed.all_gather_object(per_rank, mine)
    if rank != 0:
        return None
    state = {
        "format": FORMAT,
        "model_state_dict": model.state_dict(),
        "optimizer_state_dict": optimizer.state_dict(),
        "scheduler_state_dict": scheduler.state_dict() if scheduler is not None else None,
        "per_rank": per_rank,
        "epoch": int(epoch),
        "best_val_acc": best_val_acc,
        "no_improve_count": int(no_improve_count),
        "world_size": world,
        "param_layout": param_layout(optimizer),
        "config": state_config(config),
    }
    path = os.fspath(path)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tmp = f"{path}.tmp.{os.getpid()}"
    try:
        torch.save(state, tmp)
        os.replace(tmp, path)                         # atomic on one file system: never a partial target
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return path


PROXY_HEAD = "proxy_head.pt"


def save_proxy_head(directory, head):
    """The ``metric_loss`` head of a run (``prototypes.ProxyHead``) as ``directory/proxy_head.pt``: proxies, names, scale and
    margin -- data only, written beside the target and renamed over it like the run state.  ``best_model.pt`` keeps the
    reference's bare format; the proxies' optimizer state travels in the run state (they are its second parameter group)."""
    path = os.path.join(os.fspath(directory), PROXY_HEAD)
    tmp = path + ".tmp"
    torch.save({"proxies": head.proxies.detach().cpu(), "names": list(head.names), "scale": float(head.scale),
                "margin": float(head.margin)}, tmp)
    os.replace(tmp, path)
    return path


def load_proxy_head(directory, head):
    """Restore ``save_proxy_head``'s file into ``head`` (same class count; the resuming config's scale and margin are kept)."""
    path = os.path.join(os.fspath(directory), PROXY_HEAD)
    state = torch.load(path, map_location="cpu", weights_only=True)
    if tuple(state["proxies"].shape) != tuple(head.proxies.shape):
        raise ValueError(f"{path} holds proxies {tuple(state['proxies'].shape)}, the run's head {tuple(head.proxies.shape)}")
    with torch.no_grad():
        head.proxies.copy_(state["proxies"].to(head.proxies.device))
    head.names = [str(n) for n in state["names"]]
    return head


def load_run_state(path, model, optimizer, scheduler=None, mixup=None, config=None, rank=None, world=None, map_location=None,
                   adversary=None):
    """Put a saved run state back into fresh objects; every rank calls it and takes its own per-rank entry.  Returns
    ``{"epoch", "best_val_acc", "no_improve_count", "config", "config_changed"}`` (``epoch``: the last finished one).
    Raises ``ValueError`` -- before anything is loaded -- when the world size, the parameter layout, or the presence of a
    scheduler / mixup / adversary differs from the saved run's (a file from before ``adversary_rng`` existed had none)."""
    rank, world = _rank_world(rank, world)
    if map_location is None:
        params = [p for group in optimizer.param_groups for p in group["params"]]
        map_location = params[0].device if params else "cpu"
    state = torch.load(os.fspath(path), map_location=map_location, weights_only=False)
    if not isinstance(state, dict) or state.get("format") != FORMAT:
        raise ValueError(f"{path}: not a run state of format {FORMAT} (a bare state dict such as best_model.pt cannot be resumed)")
    if int(state["world_size"]) != world:
        raise ValueError(f"{path}: saved by a run of world size {state['world_size']}, this run has world size {world}: the "
                         "per-rank dropout, mixup and adversary state does not carry over")
    layout = param_layout(optimizer)
    if state["param_layout"] != layout:
        def brief(lay):
            return [f"{len(g)} tensors / {sum(g)} elements" for g in lay]
        raise ValueError(f"{path}: saved parameter layout {brief(state['param_layout'])} differs from this run's {brief(layout)} "
                         "(another model, label set or freeze list)")
    for name, obj, saved in (("LR scheduler", scheduler, state["scheduler_state_dict"]),
                             ("mixup", mixup, state["per_rank"][rank]["mixup_rng"]),
                             ("adversary", adversary, state["per_rank"][rank].get("adversary_rng"))):
        if (obj is None) != (saved is None):
            raise ValueError(f"{path}: the saved run had {'a' if saved is not None else 'no'} {name}, this run has "
                             f"{'one' if obj is not None else 'none'}")
    model.load_state_dict(state["model_state_dict"])
    optimizer.load_state_dict(state["optimizer_state_dict"])
    if scheduler is not None:
        scheduler.load_state_dict(state["scheduler_state_dict"])
    mine = state["per_rank"][rank]
    if mixup is not None:
        mixup.rng.setstate(mine["mixup_rng"])
    if adversary is not None:
        adversary.rng.setstate(mine["adversary_rng"])
    train_ops.set_dropout_step(mine["dropout_step"])
    saved_cfg, now = state.get("config") or {}, state_config(config)
    changed = sorted(k for k in set(saved_cfg) | set(now) if saved_cfg.get(k) != now.get(k)) if config is not None else []
    return {"epoch": int(state["epoch"]), "best_val_acc": state["best_val_acc"], "no_improve_count": int(state["no_improve_count"]),
            "config": saved_cfg, "config_changed": changed}
