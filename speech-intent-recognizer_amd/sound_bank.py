"""A set of mono clips resident in HBM as one padded tensor: the room impulse responses and the background noises of
``HipFeaturizer.reverb_mix`` (``sir_wave_reverb_mix``).

The reference has neither effect; the usual host recipe convolves one clip at a time with a RIR read from disk and adds a
noise file scaled on the CPU.  Here both banks are staged once -- a few hundred RIRs of at most 8192 taps are 3 MB, an hour
of noise at 16 kHz is 230 MB of the 288 GB -- and a training batch only carries indices into them.
"""
import os

import torch

MAX_RIR_TAPS = 8192         # what sir_wave_reverb_mix accepts (16 partitions of 512 taps)


def prepare_rir(h, max_taps=MAX_RIR_TAPS):
    """A measured or simulated impulse response as the kernel should see it: everything ahead of the direct-path peak
    (the largest |h|, the first one on a tie) is dropped so that the peak is tap 0 and the convolution does not delay the
    clip, the response is cut at ``max_taps`` taps, and it is scaled to a peak of magnitude 1 (the sign is kept)."""
    h = torch.as_tensor(h, dtype=torch.float32).reshape(-1)
    if h.numel() == 0 or not bool(torch.isfinite(h).all()):
        raise ValueError("an impulse response must be a non-empty finite vector")
    mag = h.abs()
    peak = float(mag.max())
    if peak == 0.0:
        raise ValueError("an all-zero impulse response has no direct path")
    first = int((mag == mag.max()).nonzero()[0])
    return (h[first:first + int(max_taps)] / peak).contiguous()


class SoundBank:
    """``len(bank)`` clips as ``data`` float32 ``[n, stride]`` (zero behind each clip) with ``lengths`` int32 ``[n]`` on one
    device, and ``host_lengths`` (a list) for drawing offsets without a device sync.  ``kind="rir"`` runs every clip through
    ``prepare_rir``; ``kind="noise"`` keeps the clips as they are."""

    def __init__(self, clips, device=None, kind="noise"):
        if kind not in ("noise", "rir"):
            raise ValueError("kind must be 'noise' or 'rir'")
        clips = [torch.as_tensor(c).detach().to("cpu", torch.float32).reshape(-1) for c in clips]
        if kind == "rir":
            clips = [prepare_rir(c) for c in clips]
        if not clips or any(c.numel() == 0 for c in clips):
            raise ValueError("a SoundBank needs at least one clip and no empty ones")
        self.kind = kind
        self.host_lengths = [int(c.numel()) for c in clips]
        self.max_len = max(self.host_lengths)
        stride = (self.max_len + 7) // 8 * 8                   # rows stay 32-byte aligned
        data = torch.zeros((len(clips), stride), dtype=torch.float32)
        for i, c in enumerate(clips):
            data[i, :c.numel()] = c
        device = torch.device(device) if device is not None else torch.device("cpu")
        self.data = data.to(device)
        self.lengths = torch.tensor(self.host_lengths, dtype=torch.int32, device=device)
        self._on = {}

    def __len__(self):
        return len(self.host_lengths)

    @property
    def device(self):
        return self.data.device

    def on(self, device):
        """This bank on ``device`` (staged there once and remembered)."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device == self.data.device:
            return self
        if device not in self._on:
            other = SoundBank.__new__(SoundBank)
            other.kind, other.host_lengths, other.max_len = self.kind, self.host_lengths, self.max_len
            other.data, other.lengths, other._on = self.data.to(device), self.lengths.to(device), {}
            self._on[device] = other
        return self._on[device]

    @classmethod
    def from_dir(cls, path, device=None, kind="noise", sample_rate=16000, max_seconds=None):
        """Every ``*.wav`` below ``path`` (sorted), read with the project's ``wav_io``, mixed down to mono on the host (a mean
        over channels); a file at another rate goes through ``sir_resample`` (which needs the GPU).  ``max_seconds`` cuts
        long noise files."""
        from .scripts.utils import wav_io
        files = sorted(os.path.join(d, f) for d, _, fs in os.walk(path) for f in fs if f.lower().endswith(".wav"))
        if not files:
            raise ValueError(f"no .wav files below {path}")
        clips = []
        for f in files:
            x, sr = wav_io.read_wav(f)
            x = x.mean(dim=0)
            if sr != sample_rate:
                from .featurizer import get_featurizer
                y, n = get_featurizer(sample_rate).resample(x[None, :].cuda(), sr, sample_rate)
                x = y[0, :int(n[0])].cpu()
            if max_seconds is not None:
                x = x[:int(max_seconds * sample_rate)]
            clips.append(x)
        return cls(clips, device, kind)
