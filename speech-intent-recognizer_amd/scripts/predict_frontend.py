"""``scripts/test_model.py``'s ``predict`` / ``predict_many`` for a checkpoint trained with another feature front-end.

``test_model.py`` mirrors the reference's file and keeps its surface and its front-end (1024 / 512 / 1024, 200 frames).  A
checkpoint does not record the front-end it was trained with (``best_model.pt`` is the reference's bare ``state_dict``), so the
caller hands it over here: ``frontend`` is a ``FrontEnd``, a config dict with the YAML keys ``n_fft`` / ``hop_length`` /
``win_length``, or None (= the default), and ``pad_to`` the run's ``mel_spec_length``.  Same result dictionaries, same error
convention (logged, ``None`` returned, never raised).  CLI: ``--model --label_map --config <the run's YAML> --audio <file | dir>``.
"""
import argparse
import json
import logging
import os
import sys

import torch

from sir_amd import ops
from sir_amd.frontend_config import FrontEnd, as_frontend
from sir_amd.scripts import classify_results, test_model
from sir_amd.scripts.precompute_features import AudioFeatureExtractor

logger = logging.getLogger(__name__)

_extractors = {}


def get_extractor(frontend=None):
    """The ``AudioFeatureExtractor`` of a front-end, one per front-end."""
    fe = as_frontend(frontend)
    if fe not in _extractors:
        _extractors[fe] = AudioFeatureExtractor(n_fft=fe.n_fft, hop_length=fe.hop_length, win_length=fe.win_length)
    return _extractors[fe]


def predict_many(model, audio_paths, label_map, device, pad_to=test_model.MAX_LENGTH, frontend=None, on_device=False,
                 temperature=None, min_confidence=None, slots=None, tuples=None, decode="independent", prototypes=None,
                 min_similarity=None):
    """One feature pass at ``frontend`` and one forward for all files -> list of result dictionaries / ``None``.
    ``pad_to=None`` needs a single file (un-padded features, ``T >= 8``).  ``on_device`` ... ``min_similarity`` are the
    result route, described once on ``classify_results.ResultOptions``: a wrong combination raises ``ValueError`` (a caller's
    mistake: raised, not logged), before any device call."""
    opts = classify_results.ResultOptions(on_device, temperature, min_confidence, slots, tuples, decode, prototypes, min_similarity)
    audio_paths = list(audio_paths)
    try:
        feats = get_extractor(frontend).extract_batch(audio_paths, max_duration=600.0)
        keep = [i for i, f in enumerate(feats) if f is not None]
        results = [None] * len(feats)
        if not keep:
            return results
        if pad_to is None:
            if len(keep) != 1:
                raise ValueError("pad_to=None scores one file at a time")
            batch = feats[keep[0]].unsqueeze(0).to(device)
        else:
            batch = torch.stack([test_model._pad_or_trim(feats[i].unsqueeze(0), pad_to)[0] for i in keep]).to(device)
        with torch.no_grad():
            output = model.embed(batch) if opts.embed else model(batch)
        for res, i in zip(opts.results(output, {v: k for k, v in label_map.items()}), keep):
            results[i] = res
        ops.check_status()
        return results
    except Exception as e:
        logger.error(f"Error during prediction: {str(e)}")
        return [None] * len(audio_paths)


def predict(model, audio_path, label_map, device, pad_to=test_model.MAX_LENGTH, frontend=None):
    """``test_model.predict`` at ``frontend``."""
    return predict_many(model, [audio_path], label_map, device, pad_to=pad_to, frontend=frontend)[0]


def main(argv=None):
    logging.basicConfig(level=logging.INFO, format="%(asctime)s - %(levelname)s - %(message)s",
                        handlers=[logging.StreamHandler(sys.stdout)])
    parser = argparse.ArgumentParser(description="Score audio files with a model trained at another feature front-end")
    parser.add_argument("--model", type=str, default="checkpoints/best_model.pt", help="Path to the trained model")
    parser.add_argument("--label_map", type=str, default="data/processed/label_map.json", help="Path to the label map")
    parser.add_argument("--config", type=str, required=True,
                        help="YAML config of the run that trained the model: n_fft / hop_length / win_length / mel_spec_length")
    parser.add_argument("--audio", type=str, required=True, help="An audio file or a directory of audio files")
    args = parser.parse_args(argv)
    import yaml
    with open(args.config, "r") as f:
        config = yaml.safe_load(f) or {}
    fe = FrontEnd.from_config(config)
    pad_to = int(config.get("mel_spec_length", test_model.MAX_LENGTH))
    with open(args.label_map, "r") as f:
        label_map = json.load(f)
    device = torch.device("cuda")
    model = test_model.load_model(args.model, num_classes=int(config.get("num_labels", 31)), device=device)
    if model is None:
        return 1
    if os.path.isdir(args.audio):
        files = sorted(os.path.join(args.audio, f) for f in os.listdir(args.audio) if f.endswith((".wav", ".mp3", ".flac")))
    else:
        files = [args.audio]
    for path, result in zip(files, predict_many(model, files, label_map, device, pad_to=pad_to, frontend=fe)):
        print(json.dumps({"file": path, "result": result}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
