"""Drop-in for the recogniser half of the reference's scripts/testing.py, plus its batch form for long recordings.

``IntentRecognizer(model_path, label_map_path, device)`` keeps the reference's surface (testing.py:158-281): ``predict(audio_data,
sample_rate)`` -> ``{"predicted_label", "confidence", "top_predictions"}`` (:262-266) and ``process_audio``.  What the reference
does live -- ``MicrophoneListener.listen`` (:49-143) cuts a microphone stream into utterances and calls ``predict`` on each --
``recognize_recordings`` does for many recordings at once on MI355X: ``sir_amd.segmenter.Segmenter`` finds the utterances
(``sir_vad_segment``), cuts them out (``sir_vad_gather``), ``HipFeaturizer`` turns the clip batch into features and one forward
per group of recordings scores them.  ``open_streams`` is the incremental form of the same: a ``StreamSession`` takes the audio of
many live sources piece by piece (``sir_amd.streaming.StreamSegmenter``) and scores every utterance as it ends.

Features are THIS project's training features (``sir_features_fwd``: torchaudio-style mel power, dB, whole-utterance z-norm),
not the librosa ``power_to_db(ref=np.max)`` features with the fixed -30.1 / 12.7 normalisation of testing.py:189-209 -- SURVEY.md
row 11 records that those differ from what the model was trained on.  ``MicrophoneListener`` itself, PyAudio and the saving of
recordings (hardware and file I/O) are not ported.
"""
import argparse
import json
import logging

import numpy as np
import torch

from sir_amd import ops
from sir_amd.frontend_config import as_frontend
from sir_amd.segmenter import Segmenter
from sir_amd.scripts import classify_results, test_model, test_tts_samples

logger = logging.getLogger(__name__)

MAX_LENGTH = 200                 # testing.py:230
MIN_FRAMES = test_tts_samples.MIN_FRAMES
GROUP = 32                       # recordings per segmentation call and forward
MAX_RECORDING_S = 3600.0         # a longer file is cut here
TRAINED_LENGTH = "mel_spec_length"   # ``pad_to`` default: the recogniser's own ``mel_spec_length`` (200 unless it was given another)
MAX_CLIP_S = 600.0               # un-padded scoring: a longer utterance is cut here (test_model.extract_features' bound)


class IntentRecognizer:
    def __init__(self, model_path, label_map_path, device=None, segmenter=None, frontend=None, mel_spec_length=MAX_LENGTH):
        """Load the label map and the checkpoint (testing.py:159-191; the class count comes from the checkpoint's ``fc.weight``
        as in scripts/test_tts_samples.py, where the reference hard-codes 31).  ``segmenter``: the ``Segmenter`` that
        ``recognize_recordings`` uses (default: the listener's defaults).  ``frontend`` (a ``FrontEnd``, a config dict or None =
        1024 / 512 / 1024) and ``mel_spec_length``: the front-end and frame count the checkpoint was trained with -- the
        checkpoint does not record them."""
        self.device = torch.device("cuda") if device is None else torch.device(device)
        self.model, self.label_map = test_tts_samples.load_model(model_path, label_map_path, self.device)
        self._finish(segmenter, frontend, mel_spec_length)

    @classmethod
    def from_model(cls, model, label_map, device=None, segmenter=None, frontend=None, mel_spec_length=MAX_LENGTH):
        """The recogniser around an already loaded ``CNNAudioGRU`` and label map."""
        self = cls.__new__(cls)
        self.device = torch.device("cuda") if device is None else torch.device(device)
        self.model, self.label_map = model.to(self.device).eval(), dict(label_map)
        self._finish(segmenter, frontend, mel_spec_length)
        return self

    def _finish(self, segmenter, frontend=None, mel_spec_length=MAX_LENGTH):
        self.frontend = as_frontend(frontend)
        self.mel_spec_length = int(mel_spec_length)
        self.inv_label_map = {v: k for k, v in self.label_map.items()}
        self.segmenter = segmenter if segmenter is not None else Segmenter()
        self.sample_rate = self.segmenter.sample_rate

    # ---- one utterance (testing.py:222-266) ------------------------------------------------------------------------------
    def predict(self, audio_data, sample_rate):
        """audio_data: 1-D float array in [-1, 1] (or int16 PCM) -> the result dictionary of :262-266, or ``None`` on failure.
        Pad or trim to 200 frames (:229-235), softmax, top-3."""
        try:
            wave = torch.as_tensor(np.ascontiguousarray(audio_data)).reshape(1, -1)
            if wave.dtype not in (torch.float32, torch.int16):
                wave = wave.to(torch.float32)
            fz = self.frontend.featurizer()
            wave = wave.to(self.device)
            lens = torch.tensor([wave.shape[1]], dtype=torch.int32, device=self.device)
            if int(sample_rate) != self.sample_rate:
                wave, lens = fz.resample(wave, int(sample_rate), self.sample_rate, lens)
            feats = fz(wave, lens, t_pad=self.mel_spec_length)
            with torch.no_grad():
                output = self.model(feats).cpu()
            ops.check_status()
            return test_model._result(output, self.inv_label_map)
        except Exception as e:
            logger.error(f"Error during prediction: {str(e)}")
            return None

    def process_audio(self, audio_data, sample_rate):
        """testing.py:268-281"""
        result = self.predict(audio_data, sample_rate)
        if result:
            print("\n=== INTENT RECOGNITION RESULTS ===")
            print(f"Predicted Intent: {result['predicted_label']}")
            print(f"Confidence: {result['confidence'] * 100:.2f}%")
            print("\nTop Predictions:")
            for i, pred in enumerate(result["top_predictions"]):
                print(f"  {i + 1}. {pred['label']} ({pred['probability'] * 100:.2f}%)")
            print("=" * 35)

    # ---- many long recordings --------------------------------------------------------------------------------------------
    def _load_group(self, items):
        """recordings of one group (1-D arrays / tensors at the segmenter's rate, or paths) -> (wave [n, L], lengths) on the GPU"""
        if all(isinstance(x, str) for x in items):
            ext = test_model._get_extractor()
            loaded = [ext._load(p, MAX_RECORDING_S) for p in items]
            if any(x is None for x in loaded):
                raise FileNotFoundError("a recording of this group is missing")
            keys = {(ch, sr, d.dtype) for d, ch, sr in loaded}
            if len(keys) == 1:
                (ch, sr, _), = keys
                return ext.waveforms_of_group([d for d, _, _ in loaded], ch, sr, MAX_RECORDING_S)
            parts = [ext.waveforms_of_group([d], ch, sr, MAX_RECORDING_S) for d, ch, sr in loaded]
            items = [(w[0, :int(n.item())].float() / 32768.0 if w.dtype == torch.int16 else w[0, :int(n.item())]) for w, n in parts]
        waves = [torch.as_tensor(x).reshape(-1) for x in items]
        dtype = torch.int16 if all(w.dtype == torch.int16 for w in waves) else torch.float32
        waves = [w if w.dtype == dtype else (w.float() / 32768.0 if w.dtype == torch.int16 else w.to(torch.float32)) for w in waves]
        lens = [int(w.numel()) for w in waves]
        width = (max(max(lens), 1) + 7) // 8 * 8                 # rows stay 16-byte aligned for the vector loads
        batch = torch.zeros((len(waves), width), dtype=dtype, device=self.device)
        for k, w in enumerate(waves):
            batch[k, :lens[k]] = w.to(self.device)
        return batch, torch.tensor(lens, dtype=torch.int32, device=self.device)

    def score_segments(self, wave, lengths, pad_to=TRAINED_LENGTH, logits_on_device=False, embed=False):
        """Segment a GPU batch of recordings and score every utterance -> (seg_table int32 [n, 3] on the CPU, logits [n, C] on
        the CPU).  ``pad_to`` frames: every clip is cut to fewer than ``pad_to * hop`` samples (the trim of :231-232, in samples)
        and padded to ``pad_to`` frames; ``pad_to=None``: every clip is scored at its own length through the ragged forward
        (``lengths=``), a clip with fewer than 8 frames at 8.  ``logits_on_device=True`` leaves the logits where they were
        computed (for ``classify_results.results_from_logits``).  ``embed=True``: embeddings [n, 512] instead of logits."""
        seg = self.segmenter
        if pad_to == TRAINED_LENGTH:
            pad_to = self.mel_spec_length
        table, _, total = seg.segment(wave, lengths)
        host_table = table.cpu()
        n = host_table.shape[0]
        num_classes = self.model.fc.weight.shape[0]
        if n == 0:
            return host_table, torch.zeros((0, 512 if embed else num_classes), dtype=torch.float32)
        longest = int((host_table[:, 2] - host_table[:, 1]).max())
        limit = self._clip_limit(pad_to)
        clips, clip_lens = seg.gather(wave, table, total, max(1, min(longest, limit)))
        return host_table, self._score_clips(clips, clip_lens, pad_to, logits_on_device, embed)

    def _clip_limit(self, pad_to):
        """most samples of an utterance that are scored (``pad_to`` already resolved)"""
        return self.frontend.max_samples(pad_to) if pad_to is not None else int(MAX_CLIP_S * self.segmenter.sample_rate)

    def _score_clips(self, clips, clip_lens, pad_to, logits_on_device=False, embed=False):
        """The scoring half of ``score_segments``, shared with ``StreamSession``: zero-tailed clips [n, L] and their lengths on the
        GPU -> logits [n, C]; ``pad_to`` is a frame count or None (ragged), already resolved.  ``embed=True``: the embeddings
        [n, 512] (``model.embed``) instead of the logits, for the prototype head."""
        hop = self.frontend.hop_length
        fz = self.frontend.featurizer()
        frames = (clip_lens // hop + 1).clamp(min=MIN_FRAMES)
        t_pad = pad_to if pad_to is not None else int(frames.max().item())
        feats = fz(clips, clip_lens, t_pad=t_pad)
        with torch.no_grad():
            run = self.model.embed if embed else self.model
            logits = run(feats) if pad_to is not None else run(feats, lengths=frames)
        if not logits_on_device:
            logits = logits.cpu()
        ops.check_status()
        return logits

    def recognize_recordings(self, waves_or_paths, pad_to=TRAINED_LENGTH, on_device=False, temperature=None, min_confidence=None,
                             slots=None, tuples=None, decode="independent", prototypes=None, min_similarity=None):
        """waves_or_paths: recordings as 1-D float32 / int16 arrays or tensors at the segmenter's sample rate, or paths of WAVE
        files (decoded, mixed to mono and resampled on the GPU).  -> per recording, the list of its utterances in time order:
        ``{"start": seconds, "end": seconds, "predicted_label", "confidence", "top_predictions"}``; ``None`` for the recordings of
        a group that failed (logged, as the reference's ``predict`` does).
        ``on_device`` ... ``min_similarity`` are the result route of every utterance's dictionary, described once on
        ``classify_results.ResultOptions``; a wrong combination raises ``ValueError`` before any device call.  With
        ``on_device=True`` the utterances of a group share one launch and one copy."""
        opts = classify_results.ResultOptions(on_device, temperature, min_confidence, slots, tuples, decode, prototypes, min_similarity)
        items = list(waves_or_paths)
        results = [None] * len(items)
        sr = float(self.segmenter.sample_rate)
        for g in range(0, len(items), GROUP):
            group = items[g:g + GROUP]
            try:
                wave, lens = self._load_group(group)
                table, logits = self.score_segments(wave, lens, pad_to=pad_to, logits_on_device=opts.on_device, embed=opts.embed)
                found = [[] for _ in group]
                for (r, a, b), res in zip(table.tolist(), opts.results(logits, self.inv_label_map)):
                    found[r].append({"start": a / sr, "end": b / sr, **res})
                results[g:g + len(group)] = found
            except Exception as e:
                logger.error(f"Error recognising recordings {g}..{g + len(group) - 1}: {str(e)}")
        return results

    # ---- live streams ----------------------------------------------------------------------------------------------------
    def open_streams(self, n_streams, max_push=1024, max_utterance=10.0, dtype=None, pad_to=TRAINED_LENGTH, on_device=False,
                     temperature=None, min_confidence=None, sample_rate=None, encoding=None, slots=None, tuples=None,
                     decode="independent", prototypes=None, min_similarity=None):
        """What ``MicrophoneListener.listen`` + ``predict`` do for one microphone (testing.py:49-143), for ``n_streams`` sources
        that deliver at most ``max_push`` samples of ``dtype`` (float32 unless given) per ``feed``: -> a ``StreamSession``.  The
        detector takes the listener values of this recogniser's ``segmenter``; an utterance longer than ``max_utterance`` seconds
        is ended there.  ``pad_to`` as in ``recognize_recordings``; ``on_device`` ... ``min_similarity`` are the session's
        result route (``classify_results.ResultOptions``, as there).
        ``sample_rate`` (Hz, default the segmenter's) / ``encoding`` ("pcm", "ulaw", "alaw"; default "pcm"): the callers' own rate
        and codec -- e.g. 8000 and "ulaw" for G.711 telephony, fed as bytes.  The streams are then decoded and rate-converted on
        the GPU with carried filter state (``sir_amd.streaming.StreamInput``), ``max_push`` counts the callers' samples, and
        ``start`` / ``end`` stay seconds."""
        return StreamSession(self, n_streams, max_push, max_utterance, dtype, pad_to, on_device, temperature, min_confidence,
                             sample_rate, encoding, slots, tuples, decode, prototypes, min_similarity)


class StreamSession:
    """Utterances of many live streams, scored as they end (``IntentRecognizer.open_streams``)."""

    def __init__(self, recognizer, n_streams, max_push, max_utterance, dtype, pad_to, on_device, temperature, min_confidence,
                 sample_rate=None, encoding=None, slots=None, tuples=None, decode="independent", prototypes=None, min_similarity=None):
        self.opts = classify_results.ResultOptions(on_device, temperature, min_confidence, slots, tuples, decode, prototypes,
                                                   min_similarity)
        from sir_amd.streaming import StreamSegmenter
        seg = recognizer.segmenter
        self.recognizer = recognizer
        if dtype is None and encoding in (None, "pcm"):
            dtype = torch.float32
        self.segmenter = StreamSegmenter(n_streams, max_push, max_utterance, dtype, recognizer.device, sample_rate=seg.sample_rate,
                                         chunk_size=seg.chunk_size, threshold=seg.threshold, silence_limit=seg.silence_limit,
                                         prior_recording=seg.prior_recording, flush_tail=seg.flush_tail, input_rate=sample_rate,
                                         encoding=encoding)
        self.pad_to = recognizer.mel_spec_length if pad_to == TRAINED_LENGTH else pad_to
        self.last_logits = None

    def feed(self, chunks, lengths=None, close=()):
        """chunks: ``{stream: new samples}`` -- a 1-D int16 / float array, or for G.711 streams ``bytes`` / a uint8 array of codes
        (streams not named get nothing; samples already in the session's dtype are handed through unconverted, ``bytes`` are read
        as that dtype) -- or a padded [n_streams, <= max_push] tensor with ``lengths``.  ``close``: the streams that end with this call.  -> the utterances that completed, stream-major
        then by time, as the dictionaries of ``recognize_recordings`` plus ``"stream"`` and ``"forced"`` (the utterance reached
        ``max_utterance`` and was cut there); ``start`` / ``end`` count from the stream's last close.  ``last_logits`` holds the
        logits of the utterances the latest call returned, row for row (None if there were none; with ``prototypes`` their
        embeddings)."""
        seg, reco = self.segmenter, self.recognizer
        if isinstance(chunks, dict):
            np_dtype = torch.empty(0, dtype=seg.dtype).numpy().dtype
            chunks = {s: (np.frombuffer(x, dtype=np_dtype).copy() if isinstance(x, (bytes, bytearray, memoryview)) else x)
                      for s, x in chunks.items()}
            width = max([1] + [int(np.asarray(x).size) for x in chunks.values()])
            host = torch.zeros((seg.n_streams, width), dtype=seg.dtype)
            host_len = torch.zeros((seg.n_streams,), dtype=torch.int32)
            for s, x in chunks.items():
                if not 0 <= int(s) < seg.n_streams:
                    raise ValueError(f"stream {s!r} outside [0, {seg.n_streams})")
                x = torch.as_tensor(np.ascontiguousarray(x)).reshape(-1)
                if x.dtype != seg.dtype:
                    if seg.dtype == torch.uint8:
                        raise ValueError(f"stream {s!r}: a G.711 stream is fed uint8 codes or bytes, not {x.dtype}")
                    x = x.float() / 32768.0 if x.dtype == torch.int16 else x.to(seg.dtype)
                host[int(s), :x.numel()] = x
                host_len[int(s)] = x.numel()
            chunks, lengths = host.to(reco.device), host_len.to(reco.device)
        table, total = seg.push_table(chunks, lengths, close=close if torch.is_tensor(close) else list(close))
        host_table = table.cpu()
        self.last_logits = None
        if host_table.shape[0] == 0:
            return []
        longest = int((host_table[:, 2] - host_table[:, 1]).max())
        clips, clip_lens = seg.gather(table, total, max(1, min(longest, reco._clip_limit(self.pad_to))))
        logits = self.last_logits = reco._score_clips(clips, clip_lens, self.pad_to, self.opts.on_device, self.opts.embed)
        sr = float(seg.sample_rate)
        return [{"stream": s, "forced": bool(flag & 1), "start": a / sr, "end": b / sr, **res}
                for (s, a, b, flag), res in zip(host_table.tolist(), self.opts.results(logits, reco.inv_label_map))]

    def close(self, streams):
        """End ``streams`` without new samples: their open utterances are flushed and scored, the slots start again at 0."""
        return self.feed({}, close=streams)


def main():
    parser = argparse.ArgumentParser(description="Speech intent recognition of the utterances of long recordings")
    parser.add_argument("--model", type=str, default="checkpoints/best_model.pt", help="Path to the trained model")
    parser.add_argument("--label_map", type=str, default="data/processed/label_map.json", help="Path to the label map")
    parser.add_argument("--threshold", type=float, default=0.01, help="Energy threshold for speech detection")
    parser.add_argument("--silence_limit", type=float, default=1.0, help="Seconds of silence that end an utterance")
    parser.add_argument("recordings", nargs="+", help="WAVE files to segment and recognise")
    args = parser.parse_args()
    recognizer = IntentRecognizer(args.model, args.label_map,
                                  segmenter=Segmenter(threshold=args.threshold, silence_limit=args.silence_limit))
    for path, found in zip(args.recordings, recognizer.recognize_recordings(args.recordings)):
        print(json.dumps({"file": path, "utterances": found}))


if __name__ == "__main__":
    main()
