"""Drop-in for the reference's scripts/test_tts_samples.py: score a directory of recordings and write the report files.

Same surface -- ``setup_report_folder``, ``load_model(model_path, label_map_path, device)`` (class count from ``fc.weight``,
:26-72), ``process_single_audio`` -> ``{"intent", "confidence", "top_predictions"}`` or ``None`` (:74-114),
``test_audio_files(model_path, audio_dir, label_map_path, details_csv=None, report_dir=...)`` (:116-262) and the
``--model --audio_dir --label_map --details_csv --report_dir`` CLI (:264-273), plus ``predict_many``: the un-padded scoring of many
files in ragged batches.  The reference feeds each file un-padded, at its own
length, one forward per file (:83-87); here the whole directory goes through ONE feature pass and the ragged forward
(``sir_model_infer_ragged``: mixed-length clips in one batch, each with the logits it gets on its own), in batches of at most 256.

``detailed_results.csv`` is always written; ``classification_report.csv`` and the confusion matrix (``confusion_matrix.csv``, and
``confusion_matrix.png`` when a plotting library is there) when expected labels exist.  Plots are best-effort: a missing plotting
library is logged, not raised.  The results come back as a pandas frame, or as a list of dicts on a machine without pandas.
"""
import argparse
import csv
import json
import logging
import os
import sys
from pathlib import Path

import torch

from sir_amd import ops
from sir_amd.models.models import CNNAudioGRU
from sir_amd.scripts import test_model

logger = logging.getLogger(__name__)

RESULT_COLUMNS = ("filename", "text", "expected_label", "predicted_label", "confidence", "correct", "top_predictions")


def setup_report_folder(folder_name="model_analysis"):
    """Create folder for storing report visuals (:20-24)."""
    report_dir = os.path.join("checkpoints", folder_name)
    os.makedirs(report_dir, exist_ok=True)
    return report_dir


def load_model(model_path, label_map_path, device):
    """Load model and label map; the class count comes from the checkpoint's ``fc.weight``, not the label map (:26-72)."""
    with open(label_map_path, "r") as f:
        label_map = json.load(f)
    checkpoint = torch.load(model_path, map_location=device)
    if isinstance(checkpoint, dict) and "model_state_dict" in checkpoint:
        state_dict = checkpoint["model_state_dict"]
    else:
        state_dict = checkpoint
    if "fc.weight" in state_dict:
        num_classes = state_dict["fc.weight"].shape[0]
        print(f"Detected {num_classes} classes in the model checkpoint")
    else:
        num_classes = len(label_map)
        print(f"Using {num_classes} classes from label map")
    model = CNNAudioGRU(num_classes=num_classes)
    model.load_state_dict(state_dict)
    model = model.to(device)
    model.eval()
    if len(label_map) < num_classes:
        print(f"Warning: Label map has {len(label_map)} classes, but model has {num_classes} classes.")
        print("This may cause prediction errors if the model predicts a class not in your label map.")
    return model, label_map


def _tts_result(res):
    """test_model's result -> the reference's dictionary (:97-112)"""
    if res is None:
        return None
    top = [{"rank": i + 1, "label": p["label"], "probability": p["probability"]} for i, p in enumerate(res["top_predictions"])]
    return {"intent": res["predicted_label"], "confidence": res["confidence"], "top_predictions": top}


RAGGED_BATCH = 256               # clips per ragged batch (the GRU clusters are full at multiples of 16)
MIN_FRAMES = 8                   # three 2x2 poolings: a shorter clip has no GRU step


def predict_many(model, audio_paths, label_map, device, pad_to=None):
    """Batched form of ``test_model.predict(..., pad_to=None)`` (:83-96 for many files): one feature pass, then the ragged forward
    in groups of at most ``RAGGED_BATCH`` files, each group padded to its longest clip and every clip scored at its own length
    -> list of ``test_model`` results / ``None``.  Errors follow ``test_model``: logged, ``None`` for the files of the group they hit.
    A file with fewer than ``MIN_FRAMES`` frames yields ``None`` and leaves its
    neighbours alone.  With a ``pad_to`` this is ``test_model.predict_many`` (every clip padded or cut to that length)."""
    if pad_to is not None:
        return test_model.predict_many(model, audio_paths, label_map, device, pad_to=pad_to)
    audio_paths = list(audio_paths)
    try:
        feats = test_model._get_extractor().extract_batch(audio_paths, max_duration=600.0)
    except Exception as e:
        logger.error(f"Error extracting features: {str(e)}")
        return [None] * len(audio_paths)
    results = [None] * len(feats)
    inv = {v: k for k, v in label_map.items()}
    keep = []
    for i, f in enumerate(feats):
        if f is None:
            continue
        if f.size(-1) < MIN_FRAMES:
            logger.error(f"{audio_paths[i]}: {f.size(-1)} frames, need at least {MIN_FRAMES}")
            continue
        keep.append(i)
    for g in range(0, len(keep), RAGGED_BATCH):
        group = keep[g:g + RAGGED_BATCH]
        try:                                                   # a failing group loses its own files only
            lengths = [int(feats[i].size(-1)) for i in group]
            batch = torch.stack([torch.nn.functional.pad(feats[i], (0, max(lengths) - feats[i].size(-1))) for i in group]).to(device)
            with torch.no_grad():
                output = model(batch, lengths=lengths).cpu()
            ops.check_status()                                 # (the host has waited for the logits anyway)
            for row, i in enumerate(group):
                results[i] = test_model._result(output[row:row + 1], inv)
        except Exception as e:
            logger.error(f"Error during prediction of files {g}..{g + len(group) - 1}: {str(e)}")
    return results


def process_single_audio(model, audio_path, inv_label_map, device):
    """Process a single audio file, un-padded, and return predictions (:74-114)."""
    label_map = {v: k for k, v in inv_label_map.items()}
    return _tts_result(test_model.predict(model, audio_path, label_map, device, pad_to=None))


def _read_details(audio_dir, details_csv):
    """filename -> row of details.csv (:137-155), or None"""
    path = None
    if details_csv and Path(details_csv).exists():
        path = Path(details_csv)
    elif (audio_dir / "details.csv").exists():
        path = audio_dir / "details.csv"
    if path is None:
        return None
    with open(path, newline="") as f:
        return {row["filename"]: row for row in csv.DictReader(f)}


def _write_csv(path, header, rows):
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(header)
        w.writerows(rows)


def _classification_report(expected, predicted):
    """sklearn's ``classification_report(output_dict=True)`` layout (rows: classes, accuracy, macro avg, weighted avg) computed here,
    so that the report does not depend on sklearn being installed"""
    labels = sorted(set(expected) | set(predicted))
    rows, n = [], len(expected)
    for lab in labels:
        tp = sum(1 for e, p in zip(expected, predicted) if e == lab and p == lab)
        npred = sum(1 for p in predicted if p == lab)
        nexp = sum(1 for e in expected if e == lab)
        prec = tp / npred if npred else 0.0
        rec = tp / nexp if nexp else 0.0
        f1 = 2 * prec * rec / (prec + rec) if prec + rec else 0.0
        rows.append([lab, prec, rec, f1, nexp])
    acc = sum(1 for e, p in zip(expected, predicted) if e == p) / n
    macro = [sum(r[k] for r in rows) / len(rows) for k in (1, 2, 3)]
    weighted = [sum(r[k] * r[4] for r in rows) / n for k in (1, 2, 3)]
    return rows + [["accuracy", acc, acc, acc, acc], ["macro avg"] + macro + [n], ["weighted avg"] + weighted + [n]]


def _plots(report_dir, labels, cm, results, accuracy):
    """confusion matrix, per-class accuracy and confidence histogram (:225-259) with plain matplotlib"""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    fig, ax = plt.subplots(figsize=(14, 12))
    im = ax.imshow(cm, cmap="Blues")
    fig.colorbar(im)
    for i in range(len(labels)):
        for j in range(len(labels)):
            ax.text(j, i, str(cm[i][j]), ha="center", va="center")
    ax.set_xticks(range(len(labels)))
    ax.set_xticklabels(labels, rotation=45, ha="right")
    ax.set_yticks(range(len(labels)))
    ax.set_yticklabels(labels)
    ax.set_xlabel("Predicted Label")
    ax.set_ylabel("True Label")
    ax.set_title(f"Confusion Matrix (Accuracy: {accuracy:.2f}%)")
    fig.tight_layout()
    fig.savefig(os.path.join(report_dir, "confusion_matrix.png"), dpi=150)
    per_class = {lab: [r["correct"] for r in results if r["expected_label"] == lab] for lab in labels}
    order = sorted(labels, key=lambda lab: -sum(per_class[lab]) / len(per_class[lab]))
    fig, ax = plt.subplots(figsize=(14, 8))
    ax.bar(order, [sum(per_class[lab]) / len(per_class[lab]) for lab in order])
    ax.set_xlabel("Intent Class")
    ax.set_ylabel("Accuracy")
    ax.set_title("Per-Class Accuracy")
    ax.tick_params(axis="x", rotation=45)
    ax.grid(axis="y", alpha=0.3)
    fig.tight_layout()
    fig.savefig(os.path.join(report_dir, "class_accuracy.png"), dpi=150)
    fig, ax = plt.subplots(figsize=(12, 6))
    ax.hist([[r["confidence"] for r in results if not r["correct"]], [r["confidence"] for r in results if r["correct"]]],
            bins=20, range=(0.0, 1.0), stacked=True, color=["red", "green"])
    ax.set_xlabel("Confidence")
    ax.set_ylabel("Count")
    ax.set_title("Confidence Distribution (Green: Correct, Red: Incorrect)")
    ax.grid(alpha=0.3)
    fig.tight_layout()
    fig.savefig(os.path.join(report_dir, "confidence_distribution.png"), dpi=150)
    plt.close("all")


def test_audio_files(model_path, audio_dir, label_map_path, details_csv=None, report_dir="tts_test_results"):
    """Test model on all audio files in a directory (:116-262), through the ragged path."""
    report_dir = setup_report_folder(report_dir)
    print(f"Results will be saved to: {report_dir}")
    device = torch.device("cuda")
    model, label_map = load_model(model_path, label_map_path, device)
    audio_dir = Path(audio_dir)
    audio_files = sorted(audio_dir.glob("*.wav"))
    if not audio_files:
        print(f"No audio files found in {audio_dir}")
        return None
    details = _read_details(audio_dir, details_csv)
    scored = predict_many(model, [str(p) for p in audio_files], label_map, device)
    results = []
    for audio_file, res in zip(audio_files, scored):
        result = _tts_result(res)
        if result is None:
            print(f"Failed to process audio file: {audio_file}")
            continue
        row = details.get(audio_file.name) if details else None
        expected_label = row["class"] if row else None
        results.append({"filename": audio_file.name, "text": row["text"] if row else None, "expected_label": expected_label,
                        "predicted_label": result["intent"], "confidence": result["confidence"],
                        "correct": expected_label == result["intent"] if expected_label else None,
                        "top_predictions": result.get("top_predictions", [])})
    _write_csv(os.path.join(report_dir, "detailed_results.csv"), RESULT_COLUMNS,
               [["" if r[c] is None else r[c] for c in RESULT_COLUMNS] for r in results])
    labelled = [r for r in results if r["expected_label"] is not None]
    if labelled:
        expected = [r["expected_label"] for r in labelled]
        predicted = [r["predicted_label"] for r in labelled]
        accuracy = 100.0 * sum(1 for r in labelled if r["correct"]) / len(labelled)
        print(f"\nOverall accuracy: {accuracy:.2f}%")
        _write_csv(os.path.join(report_dir, "classification_report.csv"), ["", "precision", "recall", "f1-score", "support"],
                   _classification_report(expected, predicted))
        labels = sorted(set(expected))
        index = {lab: i for i, lab in enumerate(labels)}
        cm = [[0] * len(labels) for _ in labels]
        for e, p in zip(expected, predicted):
            if p in index:                                             # (as sklearn's confusion_matrix(labels=...): others are dropped)
                cm[index[e]][index[p]] += 1
        _write_csv(os.path.join(report_dir, "confusion_matrix.csv"), [""] + labels, [[lab] + cm[i] for i, lab in enumerate(labels)])
        try:
            _plots(report_dir, labels, cm, labelled, accuracy)
        except Exception as e:  # plotting is reporting, not part of the hot path
            logger.error(f"plots skipped: {e}")
    print(f"Results and visualizations saved to: {report_dir}")
    try:
        import pandas as pd
    except ImportError:
        logger.info("pandas is not installed: returning the results as a list of dicts")
        return results
    return pd.DataFrame(results, columns=list(RESULT_COLUMNS))


def main():
    parser = argparse.ArgumentParser(description="Test model on TTS generated audio files")
    parser.add_argument("--model", type=str, required=True, help="Path to the model checkpoint")
    parser.add_argument("--audio_dir", type=str, required=True, help="Directory containing audio files")
    parser.add_argument("--label_map", type=str, required=True, help="Path to the label map JSON file")
    parser.add_argument("--details_csv", type=str, help="Path to the details CSV file (optional)")
    parser.add_argument("--report_dir", type=str, default="tts_test_results", help="Directory to save test results")
    args = parser.parse_args()
    test_audio_files(args.model, args.audio_dir, args.label_map, args.details_csv, args.report_dir)


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO, format="%(asctime)s - %(levelname)s - %(message)s", handlers=[logging.StreamHandler(sys.stdout)])
    main()
