"""Argument handling shared by the Python wrappers of the kernels that take a waveform batch (``sir_features_*``,
``sir_mix_to_mono``, ``sir_resample``, ``sir_wave_*``, ``sir_vad_*``, ``sir_stream_*``): the batch and its length vector, the
per-utterance pointers, the ``out`` tensor, the gather arguments and the scratch buffers.  Every check reads tensor metadata
only; the device check is ``_native.require_hip`` and comes first wherever a wrapper has one.
"""
import ctypes as C

import torch

from . import _native

WAVE_CODES = {torch.float32: _native.WAVE_F32, torch.int16: _native.WAVE_I16}
INT_DTYPES = frozenset((torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8))


def is_batch_layout(wave):
    return isinstance(wave, torch.Tensor) and wave.dim() == 2 and wave.stride(1) == 1


def is_length_vector(lengths, rows):
    return isinstance(lengths, torch.Tensor) and lengths.dtype in INT_DTYPES and lengths.shape == (rows,)


def check_wave(who, wave, must="wave must be [B, L]", dtypes=WAVE_CODES, rows=None, kind="waveform", refuse_empty=False):
    """Metadata of a ``[rows, L]`` batch with unit inner stride -> (SIR_WAVE_* code, rows, L).  ``must`` words the layout for
    the message; a batch of a fixed row count (``rows``: a stream push) names its one dtype there as well."""
    if not is_batch_layout(wave) or (rows is not None and wave.shape[0] != rows):
        raise _native.SirError(f"{who}: {must} with unit inner stride")
    code = dtypes.get(wave.dtype)
    if code is None:
        raise _native.SirError(f"{who}: {must} with unit inner stride" if rows is not None else
                               f"{who}: unsupported {kind} dtype {wave.dtype}")
    n, max_len = wave.shape
    if refuse_empty and (n == 0 or max_len == 0):
        raise _native.SirError(f"{who} needs a non-empty [B, L] batch")
    return code, n, max_len


def check_lengths(who, lengths, rows, per="clip"):
    """One integer count per row -> int32, contiguous (a kernel reads ``rows`` entries whatever the tensor holds)."""
    if not is_length_vector(lengths, rows):
        got = f"{lengths.numel()} for {rows} (as a 1-D integer tensor; got {lengths.dtype} {tuple(lengths.shape)})" \
            if torch.is_tensor(lengths) else f"got a {type(lengths).__name__}, not a tensor"
        raise _native.SirError(f"{who}: lengths must hold one entry per {per}: {got}")
    return (lengths if lengths.dtype == torch.int32 else lengths.to(torch.int32)).contiguous()


def check_batch(who, wave, lengths=None, per="clip", **layout):
    """The one check of a waveform batch on the GPU -> (SIR_WAVE_* code, rows, L, lengths int32 [rows] on the wave's device,
    default all L).  ``layout``: the keywords of ``check_wave``."""
    _native.require_hip(wave, lengths)
    code, rows, max_len = check_wave(who, wave, **layout)
    if lengths is None:
        return code, rows, max_len, torch.full((rows,), max_len, dtype=torch.int32, device=wave.device)
    return code, rows, max_len, check_lengths(who, lengths, rows, per)


class Keep:
    """Per-utterance arguments as device pointers.  The tensors made on the way stay referenced here, so a wrapper that holds
    its ``Keep`` in a local keeps them alive until it returns.  ``rows``: every argument must have that many values."""

    def __init__(self, device, rows=None):
        self.device, self.rows, self.held = device, rows, []

    def ptr(self, t, dtype):
        if t is None:
            return None
        t = (t if isinstance(t, torch.Tensor) else torch.as_tensor(t)).to(device=self.device, dtype=dtype).contiguous()
        if self.rows is not None and t.numel() != self.rows:
            raise _native.SirError(f"per-utterance argument of {t.numel()} values for a batch of {self.rows}")
        self.held.append(t)
        return t.data_ptr()

    def augment(self, shift, noise_sigma, noise_seed, time_mask, freq_mask):
        """``const sir_augment*`` of the feature kernels (None when nothing is drawn)"""
        if shift is None and noise_sigma is None and time_mask is None and freq_mask is None:
            return None
        aug = _native.Augment(self.ptr(shift, torch.int32), self.ptr(noise_sigma, torch.float32), int(noise_seed),
                              self.ptr(time_mask, torch.int32), self.ptr(freq_mask, torch.int32))
        return C.byref(aug)


def check_out(out, rows, cols, device, layout="[B, >= L]"):
    """``out`` as given, or a new float32 ``[rows, cols]``: float32 ``[rows, >= cols]`` with unit inner stride."""
    if out is None:
        return torch.empty((rows, cols), dtype=torch.float32, device=device)
    _native.require_hip(out)
    if out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != rows or out.shape[1] < cols or out.stride(1) != 1:
        raise _native.SirError(f"out must be float32 {layout} with unit inner stride")
    return out


def out_row_stride(out):
    """The row stride to hand the library: torch may report any stride(0) for a single row, and the library wants it to be at
    least the row's width."""
    return out.stride(0) if out.shape[0] > 1 else max(out.stride(0), out.shape[1])


def first_cols(out, cols):
    return out[:, :cols] if out.shape[1] != cols else out


def check_gather(table, total, max_clip_len, dtype, width, device):
    """Arguments of the two ``gather`` forms -> (contiguous table, max_clip_len, clips float32 [n, max_clip_len], clip lengths
    int32 [n]), the last two uninitialised."""
    _native.require_hip(table, total)
    max_clip_len = int(max_clip_len)
    if max_clip_len <= 0:
        raise _native.SirError(f"max_clip_len must be positive, got {max_clip_len}")
    if table.dtype != dtype or table.dim() != 2 or table.shape[1] != width or total.dtype != torch.int32:
        raise _native.SirError(f"table must be {str(dtype).split('.')[-1]} [n, {width}] and total int32 [1]")
    n = table.shape[0]
    return (table.contiguous(), max_clip_len, torch.empty((n, max_clip_len), dtype=torch.float32, device=device),
            torch.empty((n,), dtype=torch.int32, device=device))


class StreamScratch:
    """Grow-only scratch, one buffer per (device, stream) that calls: a workspace is live between the launches of one call (the
    dB slab of a general front-end, the stretched rows of ``sir_wave_perturb``, the gains of ``sir_wave_reverb_mix``), and
    callers such as BatchPipeline and FeaturePrefetcher run one featurizer on several streams at once.  Calls on one stream are
    ordered, so they share a buffer."""
    MIN_BYTES = 256

    def __init__(self):
        self.buffers = {}

    def get(self, nbytes, device):
        key = (device, torch.cuda.current_stream(device).cuda_stream)
        buf = self.buffers.get(key)
        if buf is None or buf.numel() < nbytes:
            # (allocated under the calling stream, so the allocator hands a replaced block to that stream only)
            buf = self.buffers[key] = torch.empty(max(int(nbytes), self.MIN_BYTES), dtype=torch.uint8, device=device)
        return buf
