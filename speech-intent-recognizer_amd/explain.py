"""Gradients of ``CNNAudioGRU`` with respect to its input features -- and, through the feature extractor, its input waveform:
saliency maps and FGSM-style robustness checks.

Everything here runs the model with EVAL semantics on the differentiable path -- all three BatchNorms on their running
statistics, no inter-layer dropout, no parameter gradient -- whatever mode the module is in, and leaves the module as it
found it: sub-module flags, running statistics, ``num_batches_tracked``, the dropout step counter, cached weight layouts
and every ``p.grad`` are untouched.  The forward is ``sir_model_train_fwd_cfg`` with ``bn_frozen = {1, 1, 1}``, the backward
``sir_model_train_bwd_emb`` with all 29 gradient pointers and ``demb`` NULL: the data chain alone, down through conv1
(``conv1_bwd_data_kernel``).  With frozen statistics the clips of a batch do not see each other, so row ``b`` of every
result is what clip ``b`` gives on its own.

The ``*_wave`` forms start from audio: features by ``sir_features_fwd`` (no augmentation), the model as above, then
``sir_features_bwd`` carries ``dx`` down to the samples.  Their ``lengths`` are SAMPLE counts of zero-padded clips (what the
featurizer takes), not the ragged model path; every clip must fit ``t_pad`` frames (``1 + L // 512 <= t_pad``).

Every call takes a training workspace of its own for as long as it needs one (``sir_amd.leases``), so it may run between a training
forward of the same model and that forward's backward; the stale-input checks of the node (``x`` or a parameter changed between
its forward and its backward: ``RuntimeError``) apply to the calls made here as well.

Arguments are validated before any device call; there is no CPU path.  Un-padded clips of mixed length have functions of their
own -- ``input_gradient_ragged``, ``saliency_ragged``, ``fgsm_ragged`` (``sir_model_train_fwd_ragged`` / ``frames`` of the backward:
row ``b`` is what clip ``b`` gives at its own length, the function ``model.eval()(x, lengths=...)`` scores); the ``lengths=``
keywords of the functions for padded batches keep raising.  ``pgd`` and the waveform forms have no ragged form.
"""
import torch

from . import _native, ops


def _frozen_cfg():
    cfg = _native.TrainConfig()
    for i in range(3):
        cfg.bn_frozen[i] = 1
    return cfg


def _on_device(model, x):
    return x.is_cuda and next(model.parameters()).is_cuda


def _require_device(model, x):
    if not _on_device(model, x):
        raise _native.SirError("tensor is not on a HIP device: this path runs on MI355X only (no CPU fallback)")


def _validate(model, x, lengths):
    if lengths is not None:
        raise ValueError("lengths= (ragged batches) is not available on the differentiable path: pass clips of one length")
    ops.check_feature_batch(x, "x", 8)
    _require_device(model, x)


def _index_vector(v, bsz, name):
    """``target`` / ``labels``: an integer tensor (or list) with one entry per clip."""
    if not torch.is_tensor(v):
        v = torch.as_tensor(list(v))
    if v.is_floating_point() or v.dtype == torch.bool:
        raise ValueError(f"{name} must be an integer tensor")
    if v.dim() != 1 or v.numel() != bsz:
        raise ValueError(f"{name} must hold one class index per clip: got shape {tuple(v.shape)} for a batch of {bsz}")
    return v


def _class_vector(model, v, bsz, name):
    """``_index_vector`` plus, for a host tensor, the range check (a device tensor is checked by the loss kernel / scatter)."""
    v = _index_vector(v, bsz, name)
    if not v.is_cuda:
        ncls = model.fc.weight.shape[0]
        bad = [(i, int(c)) for i, c in enumerate(v.tolist()) if not 0 <= int(c) < ncls]
        if bad:
            raise ValueError(f"{name} outside [0, {ncls}) (clip, class): {bad[:8]}")
    return v


def _forward(model, x, frames=None):
    """logits of the eval-semantics differentiable forward and the leaf they hang on (``x`` detached, in its own shape).
    ``frames`` (device int32 ``[B]``): the ragged step."""
    from . import train_ops
    leaf = x.detach().requires_grad_(True)
    opts = train_ops.StepOptions(cfg=_frozen_cfg(), dropout_p=0.0, step=False, frames=frames)
    with torch.enable_grad():
        # (detached parameters: the node sees no parameter that wants a gradient)
        logits = train_ops._TrainStep.apply(leaf, model, opts, *[p.detach() for p in train_ops.param_list(model)])
    return logits, leaf


def _validate_ragged(model, x, frames):
    """The checks of ``_validate`` with the clips' own lengths: shape and dtype of ``x``, then ``frames`` (one integer per clip;
    a host list or CPU tensor must lie in ``[8, T]``, a device tensor is checked by the kernels).  Returns ``frames`` as a
    tensor, still where it was; the caller checks its other arguments, then the device (``_require_device``)."""
    bsz, t = ops.check_feature_batch(x, "x", 8)
    if frames is None:
        raise ValueError("frames must hold one length per clip (for clips of one length use the function without _ragged)")
    if not torch.is_tensor(frames):
        frames = torch.as_tensor(list(frames))
    if frames.is_floating_point() or frames.dtype == torch.bool:
        raise ValueError("frames must be integers (frames per clip)")
    if frames.dim() != 1 or frames.numel() != bsz:
        raise ValueError(f"frames must hold one entry per clip: got shape {tuple(frames.shape)} for a batch of {bsz}")
    if not frames.is_cuda:
        bad = [(i, int(v)) for i, v in enumerate(frames.tolist()) if not 8 <= int(v) <= t]
        if bad:
            raise ValueError(f"frames outside [8, {t}] (clip, frames): {bad[:8]}")
    return frames


def _inside(x, frames):
    """bool ``[B, 1, T]`` (or ``[B, 1, 1, T]``): the columns of each clip below its own length."""
    m = torch.arange(x.shape[-1], device=x.device)[None, :] < frames[:, None]
    return m.view((x.shape[0],) + (1,) * (x.dim() - 2) + (x.shape[-1],))


def _input_gradient(model, x, target, ragged, frames=None, lengths=None):
    """``input_gradient`` (``lengths``: refused) and ``input_gradient_ragged`` (``frames``).  The padded form checks the device
    before ``target``, the ragged form after it."""
    if ragged:
        frames = _validate_ragged(model, x, frames)
    else:
        _validate(model, x, lengths)
    bsz = x.shape[0]
    if target is not None:
        target = _class_vector(model, target, bsz, "target")
    if ragged:
        _require_device(model, x)
        frames = frames.to(device=x.device, dtype=torch.int32).contiguous()
    logits, leaf = _forward(model, x, frames)
    if target is None:
        target = logits.detach().argmax(dim=1)
    target = target.to(device=x.device, dtype=torch.int64)
    # the backward's internal loss scale is 2^8 x batch (rounded up to a power of two), sized for the 1 / batch of a mean loss:
    # the one-hot seed carries that power of two, and the result gives it back -- both exact
    k = (bsz - 1).bit_length()
    seed = torch.zeros_like(logits).scatter_(1, target[:, None], 2.0 ** -k)
    (dx,) = torch.autograd.grad(logits, leaf, grad_outputs=seed)
    return logits.detach(), dx.mul_(2.0 ** k)


def _fgsm(model, x, labels, eps, ragged, frames=None, lengths=None):
    """``fgsm`` (``lengths``: refused) and ``fgsm_ragged`` (``frames``).  Host ``labels`` are range-checked by the ragged form
    alone: the padded form leaves them to the loss kernel."""
    from . import train_ops
    eps = float(eps)
    if not eps >= 0.0:
        raise ValueError("eps must be >= 0")
    if ragged:
        frames = _validate_ragged(model, x, frames)
        labels = _class_vector(model, labels, x.shape[0], "labels")
        _require_device(model, x)
        frames = frames.to(device=x.device, dtype=torch.int32).contiguous()
    else:
        _validate(model, x, lengths)
        labels = _index_vector(labels, x.shape[0], "labels")
    logits, leaf = _forward(model, x, frames)
    with torch.enable_grad():
        loss = train_ops.fused_cross_entropy(logits, labels.to(x.device))
    (dx,) = torch.autograd.grad(loss, leaf)
    adv = x.detach() + eps * dx.sign_()
    return torch.where(_inside(x, frames), adv, x.detach()) if ragged else adv


def input_gradient_ragged(model, x, frames, target=None):
    """``input_gradient`` for un-padded clips: row b of ``(logits, dx)`` is what ``input_gradient`` gives
    ``x[b:b+1, ..., :frames[b]]`` on its own -- the function ``model.eval()(x, lengths=frames)`` scores -- and ``dx`` is zero at
    columns ``>= frames[b]`` (``sir_model_train_fwd_ragged`` / ``frames`` of the backward).  Columns behind a clip's length are
    never read."""
    return _input_gradient(model, x, target, True, frames=frames)


def saliency_ragged(model, x, frames, target=None):
    """``saliency`` for un-padded clips: ``|dx * x|`` of ``input_gradient_ragged``, shape ``[B,64,T]``, zero at columns
    ``>= frames[b]`` whatever ``x`` holds there."""
    _, dx = input_gradient_ragged(model, x, frames, target)
    frames = torch.as_tensor(frames).to(device=x.device)
    sal = torch.where(_inside(x, frames), dx * x.detach(), torch.zeros((), device=x.device))
    return sal.abs_().view(x.shape[0], 64, x.shape[-1])


def fgsm_ragged(model, x, labels, eps, frames):
    """``fgsm`` for un-padded clips: the cross-entropy is the mean over the clips of the un-padded function's loss; columns
    ``>= frames[b]`` come back as they came, bit for bit."""
    return _fgsm(model, x, labels, eps, True, frames=frames)


def input_gradient(model, x, target=None, lengths=None):
    """``(logits, dx)`` with ``dx[b] = d logits[b, target[b]] / d x[b]`` in the shape of ``x``.  ``target``: int tensor
    ``[B]``; ``None`` = each row's own argmax.  ``logits`` are those of ``model.eval()(x)`` (detached)."""
    return _input_gradient(model, x, target, False, lengths=lengths)


def saliency(model, x, target=None, lengths=None):
    """Gradient x input, ``|dx * x|``, shape ``[B,64,T]``: which part of the spectrogram decided ``target`` (default: the
    predicted intent)."""
    _, dx = input_gradient(model, x, target, lengths)
    return (dx * x.detach()).abs_().view(x.shape[0], 64, x.shape[-1])


def fgsm(model, x, labels, eps, lengths=None):
    """The fast-gradient-sign adversarial example ``x + eps * sign(d CE(model(x), labels) / d x)`` (Goodfellow et al. 2015),
    in the shape of ``x``; the cross-entropy is the mean over the batch (``fused_cross_entropy``)."""
    return _fgsm(model, x, labels, eps, False, lengths=lengths)


def pgd(model, x, labels, eps, alpha=None, steps=10, random_start=False, seed=0, keep_zero_columns=False, lengths=None):
    """The projected-gradient-descent adversarial example (Madry et al. 2018) inside the L-infinity ball of radius ``eps`` around
    ``x``, in the shape of ``x``: ``steps`` iterations of ``clamp(x_k + alpha * sign(d CE(model(x_k), labels) / d x_k), x - eps,
    x + eps)``, each one eval-semantics forward / data-only backward (``_forward``) and ONE ``sir_adv_step`` launch; with
    ``random_start`` the first iterate is ``x + eps * (2 U - 1)`` keyed by ``seed``.  ``alpha=None``: ``train_ops.default_adv_alpha``.
    ``keep_zero_columns``: all-zero frame columns of ``x`` (padding) stay zero.  ``pgd(steps=1, alpha=eps)`` returns the bits of
    ``fgsm``."""
    from . import train_ops
    eps, steps = float(eps), int(steps)
    if not eps >= 0.0:
        raise ValueError("eps must be >= 0")
    if steps < 1:
        raise ValueError("steps must be >= 1")
    alpha = train_ops.default_adv_alpha(eps, steps, bool(random_start)) if alpha is None else float(alpha)
    if not alpha >= 0.0:
        raise ValueError("alpha must be >= 0")
    seed = int(seed)
    if not 0 <= seed < (1 << 64):
        raise ValueError("seed must fit 64 bits")
    _validate(model, x, lengths)
    labels = _index_vector(labels, x.shape[0], "labels").to(x.device)
    x0 = x.detach().contiguous()
    cur = x0
    if random_start:
        cur = train_ops.adv_step(x0, None, None, eps, alpha, seed=seed, keep_zero_columns=keep_zero_columns)
    for _ in range(steps):
        logits, leaf = _forward(model, cur)
        with torch.enable_grad():
            loss = train_ops.fused_cross_entropy(logits, labels)
        (dx,) = torch.autograd.grad(loss, leaf)
        cur = train_ops.adv_step(x0, cur, dx, eps, alpha, keep_zero_columns=keep_zero_columns, out=None if cur is x0 else cur)
    return cur


def robust_accuracy(model, x, labels, eps, **pgd_kw):
    """``(clean_correct, adversarial_correct)``: how many clips of the batch the model (eval semantics, ``model.predict``) gets
    right as they are and after ``pgd(model, x, labels, eps, **pgd_kw)``, as device int64 scalars (no host sync)."""
    x_adv = pgd(model, x, labels, eps, **pgd_kw)
    labels = _index_vector(labels, x.shape[0], "labels").to(x.device)
    _, clean = model.predict(x.detach())
    clean = (clean == labels).sum()
    _, adv = model.predict(x_adv)
    return clean, (adv == labels).sum()


# ---- down to the waveform -------------------------------------------------------------------------------------------------
def _validate_wave(model, wave, lengths, t_pad):
    from . import featurizer
    if not torch.is_tensor(wave) or wave.dtype != torch.float32 or wave.dim() != 2 or wave.shape[0] < 1 or wave.shape[1] < 1:
        raise ValueError("wave must be a float32 tensor [B, L] (dequantise PCM16 first: wave.float() / 32768)")
    t_pad = int(t_pad)
    if t_pad < 8 or 1 + wave.shape[1] // featurizer.HOP > t_pad:
        raise ValueError(f"clips of {wave.shape[1]} samples have {1 + wave.shape[1] // featurizer.HOP} frames: t_pad must be "
                         f"at least that and >= 8 (got {t_pad})")
    if lengths is not None:
        lengths = _index_vector(lengths, wave.shape[0], "lengths")
    _require_device(model, wave)
    return lengths.to(device=wave.device, dtype=torch.int32) if lengths is not None else None, t_pad


def _wave_features(wave, lengths, t_pad):
    from . import featurizer
    fz = featurizer.get_featurizer()
    wave = wave.detach().contiguous()
    db = torch.empty((wave.shape[0], fz.n_mels, t_pad), dtype=torch.float32, device=wave.device)
    return fz, wave, fz(wave, lengths, t_pad=t_pad, db_out=db), db


def wave_gradient(model, wave, lengths=None, target=None, t_pad=200, **reverb_kw):
    """``(logits, dwave)`` with ``dwave[b] = d logits[b, target[b]] / d wave[b]``, float32 ``[B, L]``, zero from ``lengths[b]``
    on: ``input_gradient`` of the clip's features, carried through the feature extractor (``sir_features_bwd``).  The arguments
    of ``HipFeaturizer.reverb_mix`` are rejected with ``ValueError``: there is no gradient through the convolution."""
    from .featurizer import reject_reverb_args
    reject_reverb_args(reverb_kw, "wave_gradient")
    lengths, t_pad = _validate_wave(model, wave, lengths, t_pad)
    if target is not None:
        target = _class_vector(model, target, wave.shape[0], "target")
    fz, wave, feats, db = _wave_features(wave, lengths, t_pad)
    logits, dx = input_gradient(model, feats, target)
    return logits, fz.features_bwd(wave, lengths, db, dx, t_pad=t_pad)


def fgsm_wave(model, wave, labels, eps, lengths=None, t_pad=200, clamp=(-1.0, 1.0), **reverb_kw):
    """The fast-gradient-sign example on the audio itself: ``clamp(wave + eps * sign(d CE(model(features(wave)), labels) / d
    wave))``; samples at or beyond ``lengths[b]`` are returned as they came.  ``clamp=None``: no clamp.  The arguments of
    ``HipFeaturizer.reverb_mix`` are rejected with ``ValueError``."""
    from .featurizer import reject_reverb_args
    reject_reverb_args(reverb_kw, "fgsm_wave")
    eps = float(eps)
    if not eps >= 0.0:
        raise ValueError("eps must be >= 0")
    if clamp is not None:
        lo, hi = (float(c) for c in clamp)
        if not lo <= hi:
            raise ValueError("clamp must be (low, high) with low <= high, or None")
    lengths, t_pad = _validate_wave(model, wave, lengths, t_pad)
    labels = _class_vector(model, labels, wave.shape[0], "labels")
    from . import train_ops
    fz, wave, feats, db = _wave_features(wave, lengths, t_pad)
    logits, leaf = _forward(model, feats)
    with torch.enable_grad():
        loss = train_ops.fused_cross_entropy(logits, labels.to(wave.device))
    (dx,) = torch.autograd.grad(loss, leaf)
    adv = wave + eps * fz.features_bwd(wave, lengths, db, dx, t_pad=t_pad).sign_()
    if clamp is not None:
        adv.clamp_(lo, hi)
    if lengths is not None:
        inside = torch.arange(wave.shape[1], device=wave.device)[None, :] < lengths[:, None]
        adv = torch.where(inside, adv, wave)
    return adv
