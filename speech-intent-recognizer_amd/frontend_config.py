"""The feature front-end of a run -- ``n_fft``, ``hop_length``, ``win_length`` (torchaudio's own names) -- read ONCE from the YAML
config and handed to every place that builds a featurizer, counts frames or names a feature cache.

Defaults: 1024 / 512 / ``n_fft`` (the reference's MelSpectrogram call).  The standard speech front-end of 25 ms / 10 ms at 16 kHz
is ``n_fft: 512, win_length: 400, hop_length: 160``; 3 s at hop 160 is 301 frames, so set ``mel_spec_length`` (the model's
``t_pad``) accordingly.  The keys are NOT stored in ``best_model.pt`` (the bare ``state_dict`` format is the reference's): they
must accompany the checkpoint.  No HIP call happens here (safe in DataLoader workers and on a host without a GPU).
"""
from collections import namedtuple

SUPPORTED_N_FFT = (256, 512, 1024)
KEYS = ("n_fft", "hop_length", "win_length")


class FrontEnd(namedtuple("FrontEnd", KEYS)):
    __slots__ = ()

    def __new__(cls, n_fft=1024, hop_length=512, win_length=None):
        n_fft, hop_length = int(n_fft), int(hop_length)
        win_length = n_fft if win_length is None else int(win_length)
        if n_fft not in SUPPORTED_N_FFT or not n_fft // 16 <= hop_length <= n_fft or not 1 <= win_length <= n_fft:
            raise ValueError(f"front-end n_fft={n_fft} hop_length={hop_length} win_length={win_length} is not built; supported: "
                             f"n_fft in {SUPPORTED_N_FFT}, n_fft/16 <= hop_length <= n_fft, 1 <= win_length <= n_fft")
        return super().__new__(cls, n_fft, hop_length, win_length)

    @classmethod
    def from_config(cls, config=None):
        """The three keys of a YAML config dict (missing keys / None: the defaults)."""
        config = config or {}
        n_fft = config.get("n_fft")
        hop = config.get("hop_length")
        return cls(1024 if n_fft is None else n_fft, 512 if hop is None else hop, config.get("win_length"))

    @property
    def is_default(self):
        return tuple(self) == (1024, 512, 1024)

    def num_frames(self, length):
        """Un-padded frame count of a clip of ``length`` samples (torch.stft, center=True)."""
        return 1 + int(length) // self.hop_length

    def max_samples(self, frames):
        """The longest clip that still has at most ``frames`` frames."""
        return int(frames) * self.hop_length - 1

    def cache_name(self, csv_stem):
        """File name of the feature cache of ``<csv_stem>.csv``: the reference's ``<stem>_features.pt`` for the default
        front-end, ``<stem>_features_n{n_fft}_h{hop}_w{win}.pt`` for any other, so that one is never taken for the other."""
        if self.is_default:
            return f"{csv_stem}_features.pt"
        return f"{csv_stem}_features_n{self.n_fft}_h{self.hop_length}_w{self.win_length}.pt"

    def featurizer(self, sample_rate=16000, n_mels=64):
        """The per-device cached ``HipFeaturizer`` of this front-end (a device call)."""
        from .featurizer import get_featurizer
        return get_featurizer(sample_rate, n_mels, self.n_fft, self.hop_length, self.win_length)


DEFAULT = FrontEnd()


def as_frontend(fe):
    """None -> the default; a ``FrontEnd``, a config dict or an (n_fft, hop_length[, win_length]) tuple -> ``FrontEnd``."""
    if fe is None:
        return DEFAULT
    if isinstance(fe, FrontEnd):
        return fe
    if isinstance(fe, dict):
        return FrontEnd.from_config(fe)
    return FrontEnd(*fe)
