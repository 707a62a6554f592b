"""Drop-in for /root/reference/scripts/evaluate.py::evaluate with the forward + argmax loop
(evaluate.py:74-86) on MI355X: one ``sir_model_infer`` launch sequence per batch, predictions kept
on the device until the loop ends (one device->host copy instead of one per batch).  Metrics and the
report files (evaluate.py:89-114) are unchanged stock sklearn / matplotlib.

YAML key ``device_metrics: true`` (default false) builds the report on the device instead: every batch is added to a
``sir_amd.metrics.EvalAccumulator`` behind its forward, the few kilobytes of counts come back once, and
``classification_report.txt`` (same text), ``confusion_matrix.png`` plus ``calibration.json`` (top-k accuracy, NLL, ECE / MCE, reliability table) are
written from them.  ``--fit_temperature VALID_CSV`` fits the softmax temperature on that split (``sir_temperature_fit``)
and writes ``temperature.json`` beside the checkpoint; ``--temperature_file`` reads one back for the calibration figures.
YAML key ``prototypes: bank.npz`` (``scripts/enroll.py`` writes one) also writes ``prototype_metrics.json``: top-1 / top-3 of the
prototype head on the split beside the ``fc`` head's (``prototype_metrics_file``)."""
import argparse
import json
import logging
import os

import torch
import yaml
from torch.utils.data import DataLoader
from tqdm import tqdm

from sir_amd import _native
from sir_amd.models.models import CNNAudioGRU
from sir_amd.scripts.dataset import FSCIntentDataset
from sir_amd.scripts.train import collate_fn, loader_kwargs

logging.basicConfig(level=logging.INFO, format="%(asctime)s - %(levelname)s - %(message)s")
logger = logging.getLogger(__name__)


def load_config(config_path):
    with open(config_path, "r") as f:
        return yaml.safe_load(f)


def load_checkpoint(model_path, num_classes, device):
    """A checkpoint (the reference's bare ``state_dict``, or a training checkpoint's ``model_state_dict``) in a
    ``CNNAudioGRU(num_classes)`` on ``device``."""
    model = CNNAudioGRU(num_classes=num_classes).to(device)
    state = torch.load(model_path, map_location=device)
    if isinstance(state, dict) and "model_state_dict" in state:
        state = state["model_state_dict"]
    model.load_state_dict(state)
    return model


def build_loader(csv_path, config, frontend, label_map_path=None, slot_spec=None):
    """The evaluation loader of a CSV split (not shuffled, no augmentation) from the run's config keys and its front-end; the
    labels come from the label map, or from ``slot_spec`` as [G] rows."""
    dataset = FSCIntentDataset(csv_path=csv_path, label_map_path=label_map_path, is_training=False,
                               use_cache=config.get("use_feature_cache", True),
                               cache_dir=config.get("cache_dir", "data/cached_features"),
                               mel_spec_length=int(config.get("mel_spec_length", 200)),
                               n_fft=frontend.n_fft, hop_length=frontend.hop_length, win_length=frontend.win_length,
                               slot_spec=slot_spec)
    return DataLoader(dataset, batch_size=config.get("batch_size", 32), shuffle=False, collate_fn=collate_fn,
                      **loader_kwargs(config.get("num_workers", 4)))


def results_dir_of(config):
    results_dir = os.path.join(config["save_path"], "evaluation_results")
    os.makedirs(results_dir, exist_ok=True)
    return results_dir


def write_report(results_dir, name, headline, text):
    """``name`` in ``results_dir``: the headline, a blank line, the report's text."""
    with open(os.path.join(results_dir, name), "w") as f:
        f.write(f"{headline}\n\n")
        f.write(text)


@torch.no_grad()
def predict_loader(model, loader, device, device_metrics=None, collect_logits=False):
    """argmax predictions and labels over a loader (the hot loop of evaluate.py:79-86).

    ``device_metrics`` (a dict of ``EvalAccumulator`` arguments: ``num_classes``, optionally ``n_bins``, ``inv_temperature``):
    every batch is also added to an accumulator on the device -- one per pipeline slot, so that the updates of a slot are
    ordered on its stream; the slots' states are merged on the host at the end -- and the result is
    ``(None, None, state arrays)``: no prediction leaves the device and no per-batch synchronisation is added.
    ``collect_logits=True`` returns ``(logits [N, C] on the device, labels [N] on the device)`` instead (for
    ``metrics.fit_temperature``).  A ``device_metrics`` dict with the key ``spec`` (a ``slots.SlotSpec``) makes the
    accumulators ``slots.SlotEvalAccumulator``s: labels are then [B, G] and the state holds the slots' states and the joint block;
    with the further key ``tuples`` (a ``slots.TupleTable``) every batch is also decoded over that table
    (``slots.ConstrainedEvalAccumulator``) and the state gains the key ``constrained``."""
    from sir_amd import metrics, ops, slots
    from sir_amd.pipeline import BatchPipeline
    from sir_amd.scripts.train import HostStager
    model.eval()
    pipe = BatchPipeline(model, n_streams=2)          # consecutive batches alternate over two HIP streams
    stage = HostStager(device, slots=4)               # host batches: persistent pinned ring (see HostStager)
    on_host = device_metrics is None and not collect_logits
    accs = cons = None
    if device_metrics is not None:
        device_metrics = dict(device_metrics)
        table = device_metrics.pop("tuples", None)
        if "spec" in device_metrics:
            accumulator = slots.SlotEvalAccumulator
            if table is not None:
                cons = [slots.ConstrainedEvalAccumulator(table=table, **device_metrics) for _ in range(pipe.n)]
        else:
            accumulator = metrics.EvalAccumulator
        accs = [accumulator(**device_metrics) for _ in range(pipe.n)]
    outputs, labels = [], []              # the host route's predictions, or the logits ``collect_logits`` asks for

    def keep_predictions(slot, out, label):
        outputs.append(out[1])
        labels.append(label)

    def accumulate(slot, out, label):
        lab = label.to(device=device, dtype=torch.int64, non_blocking=True)
        if accs is not None:
            accs[slot].update(out[0], lab)
        if cons is not None:
            cons[slot].update(out[0], label)              # (the host labels: the table rows are looked up there)
        if collect_logits:
            outputs.append(out[0])
            labels.append(lab)

    take = keep_predictions if on_host else accumulate
    for i, (mel, label) in enumerate(tqdm(loader, desc="Evaluating")):
        if mel is None or label is None or mel.size(0) == 0:
            continue                      # the reference would crash here (evaluate.py:81); skip instead
        pipe.infer(i, stage(mel), then=lambda slot, out, label=label: take(slot, out, label))
    if on_host and not outputs:
        return [], []
    pipe.synchronize()
    ops.check_status()                    # a timed-out GRU recurrence (invalid predictions), or a label outside the classes: raise
    if on_host:
        return torch.cat(outputs).cpu().numpy(), torch.cat(labels).numpy()
    if collect_logits:
        if not outputs:
            return None, None
        return torch.cat(outputs), torch.cat(labels)
    merge = slots.merge if isinstance(accs[0], slots.SlotEvalAccumulator) else metrics.merge
    state = accs[0].state_arrays()
    for a in accs[1:]:
        state = merge(state, a.state_arrays())
    if cons is not None:
        state["constrained"] = cons[0].state_arrays()
        for c in cons[1:]:
            state["constrained"] = slots.merge_constrained(state["constrained"], c.state_arrays())
    return None, None, state


def fit_temperature_file(model, loader, device, out_path, source=None, iters=20):
    """Fit beta = 1 / T on a loader's split and write ``temperature.json`` -> the dict written."""
    from sir_amd.metrics import fit_temperature
    logits, labels = predict_loader(model, loader, device, collect_logits=True)
    if logits is None:
        raise _native.SirError("fit_temperature: the split holds no usable batch")
    beta, nll_before, nll_after = (float(v) for v in fit_temperature(logits, labels, iters=iters).cpu().tolist())
    from sir_amd import ops
    ops.check_status()
    info = {"inv_temperature": beta, "temperature": 1.0 / beta, "nll_before": nll_before, "nll_after": nll_after,
            "n": int(logits.shape[0]), "iters": int(iters), "source": source}
    with open(out_path, "w") as f:
        json.dump(info, f, indent=2)
    logger.info(f"Fitted temperature T = {info['temperature']:.4f} (NLL {nll_before:.4f} -> {nll_after:.4f}); wrote {out_path}")
    return info


def read_temperature_file(path):
    """``temperature.json`` -> inv_temperature (beta = 1 / T), validated."""
    with open(path, "r") as f:
        info = json.load(f)
    beta = float(info["inv_temperature"])
    if not (beta > 0.0 and beta != float("inf")):
        raise ValueError(f"{path}: inv_temperature {beta!r} is not a positive finite number")
    return beta


def evaluate_slots(args, config):
    """``slots: {columns, map, weights}`` together with ``device_metrics: true``: the checkpoint's logit row is read as slot
    heads (sir_amd/slots.py).  Writes one ``classification_report_<column>.txt`` and ``calibration_<column>.json`` per slot
    and ``joint_metrics.json`` (exact-match accuracy, joint NLL / ECE / MCE, slots_correct, n_excluded) and returns the
    exact-match accuracy.  ``slots.map`` must name the ``slot_map.json`` of the training run: the test split's own values
    would give another class order.
    ``slots.tuples`` (the ``slot_tuples.json`` a ``slots.TupleTable`` saved) adds constrained decoding over that table:
    ``constrained_metrics.json`` (exact match under constrained decoding and the mean ``valid_mass``; for a table of at most 64
    rows also NLL / ECE / MCE of the posterior over the table) and, for such a table, ``classification_report_intents.txt``."""
    from sir_amd import metrics, slots
    opts = config["slots"]
    if not config.get("device_metrics", False):
        raise ValueError("`slots` needs `device_metrics: true` (the sklearn route knows one label per clip)")
    if not isinstance(opts, dict) or not opts.get("map"):
        raise ValueError("`slots.map` must name the slot_map.json of the training run")
    spec = slots.SlotSpec.load(opts["map"])
    table = slots.TupleTable.load(opts["tuples"], spec) if opts.get("tuples") else None
    if config.get("num_labels", spec.total) != spec.total:
        raise ValueError(f"num_labels is {config['num_labels']}, the slot layout {dict(zip(spec.columns, spec.sizes))} needs {spec.total}")
    _native.require_hip()
    from sir_amd.dist_utils import limit_host_threads
    from sir_amd.frontend_config import FrontEnd
    limit_host_threads(reserve=int(config.get("num_workers", 4)))
    device = torch.device("cuda", torch.cuda.current_device())
    model = load_checkpoint(args.model_path, spec.total, device)
    test_loader = build_loader(args.test_csv, config, FrontEnd.from_config(config), slot_spec=spec)
    _, _, arrays = predict_loader(model, test_loader, device,
                                  device_metrics={"spec": spec, "n_bins": int(config.get("calibration_bins", 15)), "tuples": table})
    results_dir = results_dir_of(config)
    for column, vocab, a in zip(spec.columns, spec.vocab, arrays["slots"]):
        report = metrics.report_from_state(a, list(vocab))
        text = metrics.format_report(report["classification"])
        logger.info(f"Slot {column}: accuracy {report['accuracy']:.4f}\n{text}")
        write_report(results_dir, f"classification_report_{column}.txt", f"Test Accuracy: {report['accuracy']:.4f}", text)
        with open(os.path.join(results_dir, f"calibration_{column}.json"), "w") as f:
            json.dump(metrics.calibration_json(report), f, indent=2)
    joint = slots.joint_report(arrays["joint"])
    with open(os.path.join(results_dir, "joint_metrics.json"), "w") as f:
        json.dump(slots.joint_json(joint), f, indent=2)
    if table is not None:
        cons, text = slots.constrained_json(arrays["constrained"], table)
        with open(os.path.join(results_dir, "constrained_metrics.json"), "w") as f:
            json.dump(cons, f, indent=2)
        if text is not None:
            write_report(results_dir, "classification_report_intents.txt",
                         f"Exact-match accuracy (constrained): {cons['exact_match_accuracy']:.4f}", text)
        logger.info(f"Constrained to {len(table)} tuples: exact-match accuracy {cons['exact_match_accuracy']:.4f} over {cons['n']} clips, "
                    f"mean valid mass {cons['mean_valid_mass']:.4f}")
    logger.info(f"Exact-match accuracy {joint['exact_match_accuracy']:.4f} over {joint['n']} clips ({joint['n_excluded']} excluded), "
                f"joint NLL {joint['nll']:.4f}, ECE {joint['ece']:.4f}")
    logger.info(f"Evaluation results saved to {results_dir}")
    return joint["exact_match_accuracy"]


def prototype_metrics_file(model, loader, device, bank_path, inv_label_map, out_path):
    """YAML key ``prototypes: bank.npz`` (a ``sir_amd.prototypes.PrototypeBank`` file, ``scripts/enroll.py`` writes one): top-1 and
    top-3 accuracy of the prototype head on the split, beside the ``fc`` head's figures from the same forward passes
    (``sir_model_embed`` with logits), written to ``prototype_metrics.json``.  A clip counts for the prototype head when its
    label's name is among the bank's classes' first k; clips whose label the bank does not know are counted (``n_unknown``)
    and miss."""
    from sir_amd import ops
    from sir_amd.prototypes import PrototypeBank
    bank = PrototypeBank.load(bank_path)
    model.eval()
    n = unknown = 0
    hits = {"prototypes": [0, 0], "fc": [0, 0]}
    for mel, label in loader:
        if mel is None or label is None or mel.size(0) == 0:
            continue
        emb, logits, _ = ops.model_embed(model, mel.to(device), model._ws, want_logits=True)
        k = min(3, int(logits.shape[1]))
        fc_idx, _ = ops.classify(logits, k=k)
        proto_idx = bank.score(emb, k=3).classes
        names = [inv_label_map.get(int(v)) for v in label.tolist()]
        want = torch.tensor([bank._index.get(name, -2) for name in names], dtype=torch.int32, device=device)
        unknown += int((want < 0).sum().item())
        for key, idx, truth in (("prototypes", proto_idx, want), ("fc", fc_idx, label.to(device).to(torch.int32))):
            hit = idx == truth[:, None]
            hits[key][0] += int(hit[:, 0].sum().item())
            hits[key][1] += int(hit.any(dim=1).sum().item())
        n += int(label.numel())
    ops.check_status()
    out = {"n": n, "n_unknown": unknown, "bank": os.path.basename(bank_path), "bank_classes": len(bank.names),
           "prototypes": {"top1": hits["prototypes"][0] / max(n, 1), "top3": hits["prototypes"][1] / max(n, 1)},
           "fc": {"top1": hits["fc"][0] / max(n, 1), "top3": hits["fc"][1] / max(n, 1)}}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=2)
    logger.info(f"Prototype head: top-1 {out['prototypes']['top1']:.4f}, top-3 {out['prototypes']['top3']:.4f} "
                f"(fc head: {out['fc']['top1']:.4f} / {out['fc']['top3']:.4f}) -> {out_path}")
    return out


def evaluate(args, config):
    if config.get("slots"):
        if config.get("prototypes"):
            raise ValueError("`prototypes` and `slots` are two different heads: evaluate one of them")
        return evaluate_slots(args, config)
    _native.require_hip()
    from sir_amd.dist_utils import limit_host_threads
    limit_host_threads(reserve=int(config.get("num_workers", 4)))
    device = torch.device("cuda", torch.cuda.current_device())
    logger.info(f"Using device: {device}")
    with open(args.label_map, "r") as f:
        label_map = json.load(f)
    inv_label_map = {v: k for k, v in label_map.items()}
    num_classes = len(label_map)
    model = load_checkpoint(args.model_path, 31, device)    # 31-way head of the shipped model (evaluate.py:45)
    logger.info(f"Loaded model from {args.model_path}")
    from sir_amd.frontend_config import FrontEnd
    fe = FrontEnd.from_config(config)       # the checkpoint does not record its front-end: the keys must accompany it
    test_loader = build_loader(args.test_csv, config, fe, args.label_map)
    inv_temperature = None
    if getattr(args, "fit_temperature", None):
        valid_loader = build_loader(args.fit_temperature, config, fe, args.label_map)
        out_path = os.path.join(os.path.dirname(os.path.abspath(args.model_path)), "temperature.json")
        inv_temperature = fit_temperature_file(model, valid_loader, device, out_path,
                                               source=os.path.basename(args.fit_temperature))["inv_temperature"]
    if getattr(args, "temperature_file", None):
        inv_temperature = read_temperature_file(args.temperature_file)
    logger.info("Starting evaluation...")
    if config.get("prototypes"):
        prototype_metrics_file(model, test_loader, device, config["prototypes"], inv_label_map,
                               os.path.join(config["save_path"], "evaluation_results", "prototype_metrics.json"))
    if config.get("device_metrics", False):
        return _evaluate_on_device(model, test_loader, device, config, inv_label_map, num_classes, inv_temperature)
    all_preds, all_labels = predict_loader(model, test_loader, device)

    from sklearn.metrics import accuracy_score, classification_report, confusion_matrix
    accuracy = accuracy_score(all_labels, all_preds)
    logger.info(f"Test Accuracy: {accuracy:.4f}")
    labels_idx = list(range(num_classes))
    target_names = [inv_label_map[i] for i in labels_idx]
    cls_report = classification_report(all_labels, all_preds, labels=labels_idx, target_names=target_names,
                                       zero_division=0)
    logger.info(f"Classification Report:\n{cls_report}")
    cm = confusion_matrix(all_labels, all_preds, labels=labels_idx)
    results_dir = results_dir_of(config)
    write_report(results_dir, "classification_report.txt", f"Test Accuracy: {accuracy:.4f}", cls_report)
    _plot_confusion(cm, target_names, results_dir)
    logger.info(f"Evaluation results saved to {results_dir}")
    return accuracy


def _plot_confusion(cm, target_names, results_dir):
    """``confusion_matrix.png`` of evaluate.py:100-114, for both routes."""
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        from sklearn.metrics import ConfusionMatrixDisplay
        plt.figure(figsize=(10, 8))
        ConfusionMatrixDisplay(confusion_matrix=cm, display_labels=target_names).plot(xticks_rotation=45)
        plt.tight_layout()
        plt.savefig(os.path.join(results_dir, "confusion_matrix.png"))
        plt.close("all")
    except Exception as e:  # plotting is reporting, not part of the hot path
        logger.error(f"confusion matrix plot skipped: {e}")


def _evaluate_on_device(model, test_loader, device, config, inv_label_map, num_classes, inv_temperature):
    """The report of ``evaluate`` from an ``EvalAccumulator`` state: the same log lines, ``classification_report.txt`` and
    ``confusion_matrix.png``, plus ``calibration.json``.  The model's head may be wider than the label map (31 classes, evaluate.py:45): the state
    covers the head, the report the label map's classes, as ``classification_report(labels=...)`` does."""
    from sir_amd import metrics
    head = model.fc.weight.shape[0]
    _, _, state = predict_loader(model, test_loader, device,
                                 device_metrics={"num_classes": head, "n_bins": int(config.get("calibration_bins", 15)),
                                                 "inv_temperature": inv_temperature})
    report = metrics.report_from_state(state)
    accuracy = report["accuracy"]
    logger.info(f"Test Accuracy: {accuracy:.4f}")
    labels_idx = list(range(num_classes))
    target_names = [inv_label_map[i] for i in labels_idx]
    cls_report = metrics.format_report(metrics.classification_from_confusion(state["confusion"], target_names, labels=labels_idx))
    logger.info(f"Classification Report:\n{cls_report}")
    results_dir = results_dir_of(config)
    write_report(results_dir, "classification_report.txt", f"Test Accuracy: {accuracy:.4f}", cls_report)
    calib =metrics.calibration_json(report)
    calib["inv_temperature"] = 1.0 if inv_temperature is None else float(inv_temperature)
    with open(os.path.join(results_dir, "calibration.json"), "w") as f:
        json.dump(calib, f, indent=2)
    # the label map's block of the matrix: what confusion_matrix(labels=labels_idx) holds on the default route
    _plot_confusion(state["confusion"][:num_classes, :num_classes], target_names, results_dir)
    logger.info(f"Top-3 accuracy {report['top3']:.4f}, NLL {report['nll']:.4f}, ECE {report['ece']:.4f}, MCE {report['mce']:.4f}")
    logger.info(f"Evaluation results saved to {results_dir}")
    return accuracy


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description="Evaluate speech intent recognition model")
    parser.add_argument("--config", type=str, required=True, help="Path to config file")
    parser.add_argument("--test_csv", type=str, required=True, help="Path to test CSV file")
    parser.add_argument("--label_map", type=str, required=True, help="Path to label map JSON file")
    parser.add_argument("--model_path", type=str, required=True, help="Path to trained model")
    parser.add_argument("--fit_temperature", type=str, default=None, metavar="VALID_CSV",
                        help="Fit the softmax temperature on this split and write temperature.json beside the checkpoint")
    parser.add_argument("--temperature_file", type=str, default=None, help="temperature.json to calibrate the confidences with")
    args = parser.parse_args()
    evaluate(args, load_config(args.config))
