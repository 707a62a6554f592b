"""Enrol intents from examples: a CSV of (path, label) -> a prototype bank file, in one forward pass per batch and no backward.

    python -m sir_amd.scripts.enroll --csv examples.csv --checkpoint best_model.pt --out bank.npz [--append bank.npz] [--exemplars]

The features are extracted exactly as ``predict_frontend.predict_many`` extracts them (the same extractor, the same ``pad_to``), so
enrolment and scoring see the same function; the files are embedded in batches (``CNNAudioGRU.embed``) and added to the bank
(``sir_amd.prototypes.PrototypeBank.enroll``: unseen labels become new classes).  ``--append`` continues a saved bank -- to the
bits of an uninterrupted enrolment; ``--exemplars`` keeps every example as a prototype of its own (1-nearest-neighbour) instead
of one mean per class.  ``--config`` names the YAML of the run that trained the checkpoint when its front-end or
``mel_spec_length`` is not the default.  Score with ``predict_frontend.predict_many(..., prototypes=PrototypeBank.load(path))``.
"""
import argparse
import csv
import logging
import sys

import torch

from sir_amd import _native, ops
from sir_amd.frontend_config import FrontEnd
from sir_amd.models.models import CNNAudioGRU
from sir_amd.prototypes import PrototypeBank
from sir_amd.scripts import predict_frontend, test_model

logger = logging.getLogger(__name__)


def read_examples(csv_path):
    """``(path, label)`` rows: a header row naming ``path`` and ``label`` columns (others are ignored), or two bare columns."""
    with open(csv_path, newline="") as f:
        rows = [r for r in csv.reader(f) if r and any(c.strip() for c in r)]
    if not rows:
        return []
    head = [c.strip().lower() for c in rows[0]]
    if "path" in head and "label" in head:
        pi, li = head.index("path"), head.index("label")
        rows = rows[1:]
    else:
        pi, li = 0, 1
    bad = [r for r in rows if len(r) <= max(pi, li) or not r[li].strip()]
    if bad:
        raise ValueError(f"{csv_path}: rows without a path and a label: {bad[:3]}")
    return [(r[pi].strip(), r[li].strip()) for r in rows]


def load_checkpoint(path, device):
    """The checkpoint's model in ``eval()``; the width of its ``fc`` head is read from the file (the head itself is not used)."""
    state = torch.load(path, map_location=device)
    if isinstance(state, dict) and "model_state_dict" in state:
        state = state["model_state_dict"]
    model = CNNAudioGRU(num_classes=int(state["fc.weight"].shape[0])).to(device)
    model.load_state_dict(state)
    return model.eval()


def enroll_files(model, examples, bank, device, pad_to=test_model.MAX_LENGTH, frontend=None, batch_size=64):
    """Embed ``examples`` (``(path, label)`` pairs) in batches and add them to ``bank`` -> (files enrolled, files that could not
    be read).  Features and padding are ``predict_many``'s."""
    extractor = predict_frontend.get_extractor(frontend)
    done = failed = 0
    for at in range(0, len(examples), batch_size):
        chunk = examples[at:at + batch_size]
        feats = extractor.extract_batch([p for p, _ in chunk], max_duration=600.0)
        keep = [i for i, f in enumerate(feats) if f is not None]
        failed += len(chunk) - len(keep)
        if not keep:
            continue
        batch = torch.stack([test_model._pad_or_trim(feats[i].unsqueeze(0), pad_to)[0] for i in keep]).to(device)
        bank.enroll(model.embed(batch), [chunk[i][1] for i in keep])
        done += len(keep)
    ops.check_status()
    return done, failed


def main(argv=None):
    logging.basicConfig(level=logging.INFO, format="%(asctime)s - %(levelname)s - %(message)s", handlers=[logging.StreamHandler(sys.stdout)])
    ap = argparse.ArgumentParser(description="Enrol intents from examples into a prototype bank")
    ap.add_argument("--csv", required=True, help="CSV of (path, label): the examples")
    ap.add_argument("--checkpoint", required=True, help="The trained model (its embeddings are enrolled; its head is not used)")
    ap.add_argument("--out", required=True, help="The bank file to write (.npz)")
    ap.add_argument("--append", default=None, help="A saved bank to continue instead of starting an empty one")
    ap.add_argument("--exemplars", action="store_true", help="Keep every example as its own prototype (1-NN) instead of class means")
    ap.add_argument("--config", default=None, help="YAML of the training run: n_fft / hop_length / win_length / mel_spec_length")
    ap.add_argument("--batch_size", type=int, default=64)
    args = ap.parse_args(argv)
    _native.require_hip()
    config = {}
    if args.config:
        import yaml
        with open(args.config, "r") as f:
            config = yaml.safe_load(f) or {}
    device = torch.device("cuda", torch.cuda.current_device())
    if args.append:
        bank = PrototypeBank.load(args.append)
        if bank.exemplars != bool(args.exemplars):
            raise ValueError(f"{args.append} is {'an exemplar' if bank.exemplars else 'a mean'} bank: --exemplars must say the same")
    else:
        bank = PrototypeBank(exemplars=args.exemplars)
    examples = read_examples(args.csv)
    done, failed = enroll_files(load_checkpoint(args.checkpoint, device), examples, bank, device,
                                pad_to=int(config.get("mel_spec_length", test_model.MAX_LENGTH)), frontend=FrontEnd.from_config(config),
                                batch_size=args.batch_size)
    bank.save(args.out)
    a = bank.state_arrays()
    logger.info(f"{done} files enrolled ({failed} unreadable, {a['skipped']} rows skipped): {len(bank.names)} classes, "
                f"{bank.n_rows} prototypes -> {args.out}")
    return 0 if done else 1


if __name__ == "__main__":
    sys.exit(main())
