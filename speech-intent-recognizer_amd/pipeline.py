"""Batch pipelining over HIP streams (torch-side wrapper of the library's ``sir_pipeline``).

The kernels of one batch run back to back on one stream; some of them cannot fill the GPU on their own (the GRU
recurrence is a chain of 25 dependent steps per layer and occupies half of the CUs at a fraction of their
matrix throughput).  Independent batches therefore alternate over a few library-owned streams, each with its OWN
feature buffer and model workspace (weights are shared, read-only): the recurrence of batch i overlaps the
convolutions of batch i+1, while the caller stays on ONE stream.  Results are bit-identical to the single-stream
path -- only the launch order across batches changes.  Measured on MI355X at batch 256: 337 k -> 410 k utterances/s.
"""
import torch

from . import _native, ops
from .featurizer import REVERB_KEYS, HipFeaturizer, get_featurizer  # noqa: F401


# sir_pipeline objects per (device, n_slots), kept for the life of the process: torch's caching allocator remembers every
# stream a tensor was record_stream()-ed on and records an event there when the tensor is freed -- a slot stream destroyed
# before that (e.g. when a BatchPipeline is garbage-collected) would be used after free at interpreter exit.
_pipelines = {}


def _library_pipeline(n):
    import ctypes as C
    key = (torch.cuda.current_device(), n)
    if key not in _pipelines:
        p = C.c_void_p()
        fz = get_featurizer()
        _native.check(_native.lib().sir_pipeline_create(fz.handle, n, C.byref(p)), "sir_pipeline_create")
        fz.pin()                           # the sir_handle must outlive the pipeline made from it
        _pipelines[key] = (p, {}, fz)      # handle, raw hipStream_t -> torch ExternalStream, the pinned featurizer
    return _pipelines[key]


class HostStager:
    """Host -> device hand-over of the batches a ``DataLoader`` yields, through a small ring of PERSISTENT pinned buffers.

    ``mel.to(device, non_blocking=True)`` (train.py:86) on what the loader hands over is the slow link of the reference-shaped
    route on this stack (devtools/dataloader_probe.py on MI355X / ROCm 7 / torch 2.10): a batch that sits in the workers'
    shared memory copies at ~50 MB/s (``pin_memory=False``: 1 k utt/s), and with ``pin_memory=True`` torch's pinning thread
    allocates a fresh pinned block per batch, which stalls for ~85 ms whenever the GPU is busy (3 k utt/s with ANY kernel in
    flight, 112 k with an idle GPU).  Here a batch is copied by the CPU into one of ``slots`` pinned buffers allocated once
    (13 MB memcpy), sent with an asynchronous copy on the caller's stream, and the buffer is reused after an event says that
    copy is done.  Tensors already on the device pass through.  (``scripts/train.py`` re-exports it.)"""

    def __init__(self, device, slots=3):
        self.device, self.slots = device, slots
        self.bufs, self.events, self.k = {}, {}, 0

    def __call__(self, t):
        if t.is_cuda:
            return t
        key = (tuple(t.shape), t.dtype)
        if key not in self.bufs:
            self.bufs[key] = [torch.empty(t.shape, dtype=t.dtype).pin_memory() for _ in range(self.slots)]
            self.events[key] = [torch.cuda.Event() for _ in range(self.slots)]
        i = self.k % self.slots
        self.k += 1
        buf, ev = self.bufs[key][i], self.events[key][i]
        ev.synchronize()                                   # (a never-recorded event returns at once)
        buf.copy_(t)
        out = buf.to(self.device, non_blocking=True)
        ev.record()
        return out


def wave_stages(fz, wave, lengths, kw):
    """The waveform stages ahead of the feature kernel, on the current stream: shift -> pitch -> speed (``sir_wave_perturb``)
    when ``kw`` carries ``pitch_cents`` / ``tempo``, then reverb -> background noise (``sir_wave_reverb_mix``) when it carries
    ``rir_index`` / ``noise_index`` -- in which case a ``shift`` goes through ``sir_wave_perturb`` too, so that it stays
    ahead of the reverb.  Returns (wave, lengths, what is left of ``kw`` for the feature kernel: Gaussian noise, SpecAugment
    and, without those stages, the shift).  Without any of those keys nothing is launched and ``kw`` comes back as it is."""
    mix = kw.get("rir_index") is not None or kw.get("noise_index") is not None
    perturb = kw.get("pitch_cents") is not None or kw.get("tempo") is not None
    if not (mix or perturb):
        return wave, lengths, kw
    kw = dict(kw)
    mix_kw = {k: kw.pop(k, None) for k in REVERB_KEYS}
    if perturb or (mix and kw.get("shift") is not None):
        wave, lengths = fz.perturb(wave, lengths, shift=kw.pop("shift", None), pitch_cents=kw.pop("pitch_cents", None),
                                   tempo=kw.pop("tempo", None))
    if mix:
        wave = fz.reverb_mix(wave, lengths, **mix_kw)
    return wave, lengths, kw


class BatchPipeline:
    """``n_streams`` slots over ``sir_pipeline`` (the LIBRARY owns the slot streams and the events that order them against
    the caller's stream -- include/sir_hip.h; this class only wraps those streams for torch's allocator and keeps one
    model workspace per slot).  ``features(i, wave, ...)`` / ``infer(i, feats)`` run batch ``i`` on the slot the library
    hands out for it; calls that carry the same ``i`` share a slot.

    Outputs of a slot are valid on the caller's stream after ``join()`` (or on the host after ``synchronize()``); a slot's
    buffers are reused ``n_streams`` batches later, so consume or copy results before that.  Results are bit-identical
    to the single-stream order."""

    def __init__(self, model, n_streams=2, frontend=None):
        _native.require_hip()
        from .frontend_config import as_frontend
        self.model = model
        self.n = max(1, int(n_streams))
        self._lib = _native.lib()
        self._p, self._ext = _library_pipeline(self.n)[:2]
        self.featurizer = as_frontend(frontend).featurizer()       # ``features`` runs this front-end (None = the default)
        self.workspaces = [model._ws] + [ops.Workspace() for _ in range(self.n - 1)]
        self._cur = None                   # (batch index, slot, torch stream) of the open submission

    def __del__(self):
        try:
            self._end()                    # never leave a slot of the shared library pipeline open
        except Exception:
            pass

    @property
    def streams(self):
        return list(self._ext.values())

    def _begin(self, i):
        """Open (or continue) the submission of batch ``i`` -> (slot, torch stream)."""
        import ctypes as C
        if self._cur is not None and self._cur[0] == i:
            return self._cur[1], self._cur[2]
        self._end()
        slot, raw = C.c_int(), C.c_void_p()
        _native.check(self._lib.sir_pipeline_begin(self._p, _native.current_stream_ptr(), C.byref(slot), C.byref(raw)),
                      "sir_pipeline_begin")
        if self.n == 1:
            st = torch.cuda.current_stream()
        else:
            st = self._ext.get(raw.value)
            if st is None:
                st = self._ext[raw.value] = torch.cuda.ExternalStream(raw.value)
        self._cur = (i, slot.value, st)
        return slot.value, st

    def _end(self):
        if self._cur is not None:
            _native.check(self._lib.sir_pipeline_end(self._p, self._cur[1]), "sir_pipeline_end")
            self._cur = None

    def slot(self, i):
        """Slot of batch ``i`` (opens its submission): index of the per-slot buffers the caller should hand over."""
        return self._begin(i)[0]

    def features(self, i, wave, lengths=None, **kw):
        k, st = self._begin(i)
        if self.n > 1:
            wave.record_stream(st)                          # must outlive the slot's kernels
            if lengths is not None:
                lengths.record_stream(st)
        with torch.cuda.stream(st):
            wave, lengths, kw = wave_stages(self.featurizer, wave, lengths, kw)
            return self.featurizer(wave, lengths, **kw)

    @torch.no_grad()
    def infer(self, i, feats, want_argmax=True, lengths=None, then=None):
        """eval-mode forward (+ argmax) of batch ``i`` on its slot's stream; closes the submission of batch ``i``.
        ``lengths`` (frames per clip): the un-padded function, as ``CNNAudioGRU.forward(x, lengths)``.
        ``then(slot, out)`` (optional) is called with the slot's stream current before the submission closes: what it
        queues (``EvalAccumulator.update`` of a per-slot accumulator, say) runs behind the forward on that stream and is
        covered by ``join()``."""
        k, st = self._begin(i)
        if self.n > 1:
            feats.record_stream(st)
            if torch.is_tensor(lengths) and lengths.is_cuda:
                lengths.record_stream(st)
        try:
            with torch.cuda.stream(st):
                out = ops.model_infer(self.model, feats, self.workspaces[k], want_argmax=want_argmax, lengths=lengths)
                if then is not None:
                    then(k, out)
        finally:
            self._end()                    # also when the forward or ``then`` raises: the shared pipeline's slot must not stay open
        return out

    def synchronize(self):
        self._end()
        self.join()
        torch.cuda.current_stream().synchronize()

    def join(self):
        """Make the caller's stream wait for every slot (no host synchronisation)."""
        self._end()
        _native.check(self._lib.sir_pipeline_join(self._p, _native.current_stream_ptr()), "sir_pipeline_join")


class FeaturePrefetcher:
    """Feature extraction one batch AHEAD of the training step, on a side stream.

    The features of the NEXT batch depend on nothing in the current training step, so the host->device copy of its
    waveforms and its feature kernels can be queued early.  (On MI355X at batch 256 with the waveforms already in HBM
    this is throughput-neutral -- 3.19 vs 3.17 ms per step: the step's kernels leave no idle CUs worth filling -- the
    point is to take the copy and the feature launch latency off the step's critical path when a loader feeds it.)
    ``submit(wave, lengths)`` queues the feature kernels of a batch into one of ``depth`` rotating buffers;
    ``get()`` makes the caller's stream wait for the oldest submitted batch and returns its ``[B, 64, t_pad]``
    buffer; ``release()`` (call it after the step that consumed the buffer has been queued -- backward reads the
    features again) lets the side stream overwrite it ``depth`` submissions later.  Values are bit-identical to the
    in-line ``HipFeaturizer`` call: same kernels, another stream."""

    def __init__(self, t_pad=200, depth=2, frontend=None, **feat_kw):
        _native.require_hip()
        from .frontend_config import as_frontend
        fe = as_frontend(frontend)
        self.t_pad, self.depth, self.kw = int(t_pad), max(2, int(depth)), feat_kw
        self.stream = torch.cuda.Stream()
        self.fz = HipFeaturizer(n_fft=fe.n_fft, hop_length=fe.hop_length, win_length=fe.win_length)
        self.bufs = [None] * self.depth
        self.ready = [torch.cuda.Event() for _ in range(self.depth)]
        self.freed = [None] * self.depth
        self.head = self.tail = 0              # next slot to fill / next slot to hand out
        self._out = None

    def submit(self, wave, lengths=None):
        if self.head - self.tail >= self.depth:
            raise RuntimeError("FeaturePrefetcher: all buffers are in flight (get() and release() first)")
        k = self.head % self.depth
        cur = torch.cuda.current_stream()
        self.stream.wait_stream(cur)                        # the waveforms are produced on the caller's stream
        wave.record_stream(self.stream)
        if lengths is not None:
            lengths.record_stream(self.stream)
        if self.freed[k] is not None:
            self.stream.wait_event(self.freed[k])           # the step that read this buffer has finished
        if self.bufs[k] is None or self.bufs[k].shape[0] != wave.shape[0]:
            self.bufs[k] = torch.empty((wave.shape[0], 64, self.t_pad), dtype=torch.float32, device=wave.device)
        with torch.cuda.stream(self.stream):
            # pitch / speed (sir_wave_perturb, with the shift), reverb / background noise (sir_wave_reverb_mix), then the
            # feature kernel with the Gaussian noise and the masks
            wave, lengths, kw = wave_stages(self.fz, wave, lengths, self.kw)
            self.fz(wave, lengths, t_pad=self.t_pad, out=self.bufs[k], **kw)
            self.ready[k].record(self.stream)
        self.head += 1

    def get(self):
        if self.tail >= self.head:
            raise RuntimeError("FeaturePrefetcher: nothing submitted")
        k = self.tail % self.depth
        torch.cuda.current_stream().wait_event(self.ready[k])
        self._out = k
        self.tail += 1
        return self.bufs[k]

    def release(self):
        """Mark the buffer handed out by the last ``get()`` as consumed by everything queued so far."""
        if self._out is None:
            return
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        self.freed[self._out] = ev
        self._out = None
