"""Result dictionaries for a whole batch, built on the device: the batch form of ``test_model._result``.

``test_model._result`` runs a softmax, an argmax, two ``.item()`` calls and a host argsort per clip.  ``results_from_logits``
makes ONE ``sir_classify`` launch and ONE device-to-host copy for all rows and returns dictionaries of the same shape.
``predict_frontend.predict_many`` and ``IntentRecognizer.recognize_recordings`` take ``on_device=True`` and come here;
``scripts/test_model.py`` and ``scripts/test_tts_samples.py`` keep their per-row route (DESIGN.md section 4 says why they
gain no keyword): their batched form is ``predict_frontend.predict_many(..., on_device=True)``, which at the default
front-end extracts the same features and runs the same forward as ``test_model.predict_many``.
"""
import numpy as np
import torch

from sir_amd import ops


def check_route(on_device, temperature, min_confidence):
    """``temperature`` and ``min_confidence`` belong to the ``on_device=True`` route of the callers: refuse them without it
    instead of dropping them silently."""
    if not on_device and (temperature is not None or min_confidence is not None):
        raise ValueError("temperature= and min_confidence= need on_device=True (the per-row host route knows neither)")


def inv_temperature_of(temperature):
    """``temperature`` of the callers (T, a positive number; None = 1) -> ``inv_temperature`` = 1 / T."""
    if temperature is None:
        return None
    t = float(temperature)
    if not (t > 0.0 and t != float("inf")):
        raise ValueError(f"temperature must be a positive finite number, got {temperature!r}")
    return 1.0 / t


def results_from_logits(logits, inv_label_map, k=3, inv_temperature=None, min_confidence=None):
    """``test_model._result`` for a whole batch: ONE ``sir_classify`` launch and ONE device-to-host copy for all rows of
    ``logits`` [B, C] -> list of B dicts of ``_result``'s shape (``top_predictions`` holds ``k`` entries, at most the number of
    classes; ``k`` above 8 is refused by ``ops.classify``).  ``inv_temperature`` (None, a number or
    ``metrics.fit_temperature``'s device scalar) calibrates the probabilities; with ``min_confidence`` set every dict also carries ``"rejected"``: the confidence is below it (or NaN)."""
    k = min(int(k), int(logits.shape[1]))
    idx, prob = ops.classify(logits, k=k, inv_temperature=inv_temperature)
    packed = torch.cat([idx.to(torch.float32), prob], dim=1).cpu().numpy()      # class indices <= 63 are exact in float32
    idx_h, prob_h = packed[:, :k].astype(np.int64), packed[:, k:]
    results = []
    for row_i, row_p in zip(idx_h.tolist(), prob_h.tolist()):
        res = {"predicted_label": inv_label_map.get(row_i[0], "Unknown"), "confidence": row_p[0],
               "top_predictions": [{"label": inv_label_map.get(i, "Unknown"), "probability": p} for i, p in zip(row_i, row_p)]}
        if min_confidence is not None:
            res["rejected"] = not (row_p[0] >= min_confidence)
        results.append(res)
    return results
