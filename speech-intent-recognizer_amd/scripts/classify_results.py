"""Result dictionaries for a whole batch, built on the device: the batch form of ``test_model._result``.

``test_model._result`` runs a softmax, an argmax, two ``.item()`` calls and a host argsort per clip.  ``results_from_logits``
makes ONE ``sir_classify`` launch and ONE device-to-host copy for all rows and returns dictionaries of the same shape.
``predict_frontend.predict_many``, ``IntentRecognizer.recognize_recordings`` and ``IntentRecognizer.open_streams`` hand their
result keywords to one ``ResultOptions`` and get their dictionaries from it;
``scripts/test_model.py`` and ``scripts/test_tts_samples.py`` keep their per-row route (DESIGN.md section 4 says why they
gain no keyword): their batched form is ``predict_frontend.predict_many(..., on_device=True)``, which at the default
front-end extracts the same features and runs the same forward as ``test_model.predict_many``.
"""
import dataclasses

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


def slot_inv_temperature_of(temperature, n_slots):
    """``temperature`` under a slot layout (None, one T for all slots, or one per slot) -> None or a list of ``1 / T``."""
    if temperature is None:
        return None
    ts = [temperature] * n_slots if isinstance(temperature, (int, float, np.floating, np.integer)) else list(temperature)
    if len(ts) != n_slots:
        raise ValueError(f"{len(ts)} temperatures for {n_slots} slots")
    return [inv_temperature_of(t) for t in ts]


def _to_host(*columns):
    """The ONE device-to-host copy of a builder: 2-D device columns [B, w] -> one float32 tensor -> one ``.cpu()`` -> the columns
    back as numpy.  An integer column travels as float32 and comes back int64: class indices and slot labels (<= 63) and
    prototype rows (<= 4095) are small integers, exact in float32."""
    packed = torch.cat([c.to(torch.float32) for c in columns], dim=1).cpu().numpy()
    out, o = [], 0
    for c in columns:
        part = packed[:, o: o + c.shape[1]]
        out.append(part if c.dtype == torch.float32 else part.astype(np.int64))
        o += c.shape[1]
    return out


def _rejected(value, threshold):
    """The ``"rejected"`` rule of every builder: below the threshold, or NaN."""
    return not (value >= threshold)


def results_from_slot_logits(logits, spec, k=3, inv_temperature=None, min_confidence=None, table=None, decode="independent"):
    """``results_from_logits`` under a slot layout (``sir_amd.slots.SlotSpec``): ONE ``sir_classify_slots`` launch and ONE
    device-to-host copy for all rows of ``logits`` [B, spec.total] -> list of B dicts: the decoded slots (``{column: value}``)
    plus ``"predicted_label"`` (``tuple_label``), ``"confidence"`` (the joint confidence: the product of the slots' top
    probabilities), ``"slot_confidence"`` (``{column: probability}``) and ``"top_predictions"`` (``{column: [{"label", "probability"}, ...]}``, ``k`` entries, at most
    the slot's width).  ``inv_temperature``: None, a number, one per slot, or ``slots.fit_slot_temperatures``' device tensor.
    With ``min_confidence`` set every dict also carries ``"rejected"``: the JOINT confidence is below it (or NaN).

    ``decode="joint"`` (ONE ``sir_decode_slots`` launch instead): the decoded slots are those of the best whole TUPLE,
    ``"confidence"`` is its probability, ``"top_predictions"`` is a list of the ``k`` best tuples (``{"label", "slots":
    {column: value}, "probability"}``), and ``min_confidence`` rejects on that confidence; there is no ``"slot_confidence"``.
    With ``table`` (a ``slots.TupleTable``) only the tuples that exist are ranked, the probabilities are the softmax over the
    table, and ``"valid_mass"`` -- the probability the independent heads put on the table, an out-of-set signal -- is added.
    A table needs ``decode="joint"``."""
    from sir_amd import slots
    k = int(k)
    check_decode(decode, table)
    if decode == "joint":
        return _joint_results(logits, spec, k, inv_temperature, min_confidence, table)
    idx, prob, joint = slots.classify(logits, spec, k=k, inv_temperature=inv_temperature)
    bsz, g = idx.shape[0], spec.n_slots
    idx_h, prob_h, joint_h = _to_host(idx.view(bsz, g * k), prob.view(bsz, g * k), joint[:, None])
    results = []
    for row_i, row_p, conf in zip(idx_h.reshape(bsz, g, k).tolist(), prob_h.reshape(bsz, g, k).tolist(), joint_h[:, 0].tolist()):
        res = spec.decode([slot_i[0] for slot_i in row_i])
        top = {}
        for c, vs, slot_i, slot_p in zip(spec.columns, spec.vocab, row_i, row_p):
            n = min(k, len(vs))
            top[c] = [{"label": vs[i] if 0 <= i < len(vs) else "Unknown", "probability": p} for i, p in zip(slot_i[:n], slot_p[:n])]
        res.update({"predicted_label": tuple_label(spec, res),
                    "confidence": conf, "slot_confidence": {c: slot_p[0] for c, slot_p in zip(spec.columns, row_p)},
                    "top_predictions": top})
        if min_confidence is not None:
            res["rejected"] = _rejected(conf, min_confidence)
        results.append(res)
    return results


def check_decode(decode, table, slots=True):
    """``decode`` is "independent" or "joint"; a tuple table belongs to joint decoding, and both to a slot layout: a caller's
    mistake is raised before any device call."""
    if decode not in ("independent", "joint"):
        raise ValueError(f'decode must be "independent" or "joint", got {decode!r}')
    if table is not None and decode != "joint":
        raise ValueError('a tuple table constrains joint decoding: pass decode="joint" with it')
    if not slots and (table is not None or decode == "joint"):
        raise ValueError("tuples= and decode=\"joint\" need a slot layout (slots=)")


def tuple_label(spec, decoded):
    """The name of a decoded tuple: the reference's ``action_object`` join when the spec has both columns, else all values
    joined by ``_``."""
    label = spec.reference_label(decoded)
    return label if label is not None else "_".join(decoded[c] for c in spec.columns)


def _joint_results(logits, spec, k, inv_temperature, min_confidence, table):
    from sir_amd import slots
    spec = slots._as_spec(spec)
    out = slots.decode(logits, spec, table=table, k=k, inv_temperature=inv_temperature, want_mass=table is not None)
    labels, prob = out[1], out[3]
    bsz, g = labels.shape[0], spec.n_slots
    host = _to_host(labels.view(bsz, k * g), prob, *([out[4][:, None]] if table is not None else []))
    lab_h, prob_h = host[0].reshape(bsz, k, g).tolist(), host[1].tolist()
    mass_h = host[2][:, 0].tolist() if table is not None else None
    results = []
    for b, (row_l, row_p) in enumerate(zip(lab_h, prob_h)):
        res = spec.decode(row_l[0])
        top = []
        for tup, p in zip(row_l, row_p):
            if tup[0] < 0 and p == 0.0:                                                   # a rank that does not exist
                continue
            d = spec.decode(tup)
            top.append({"label": tuple_label(spec, d), "slots": d, "probability": p})
        res.update({"predicted_label": tuple_label(spec, res), "confidence": row_p[0], "top_predictions": top})
        if mass_h is not None:
            res["valid_mass"] = mass_h[b]
        if min_confidence is not None:
            res["rejected"] = _rejected(row_p[0], min_confidence)
        results.append(res)
    return results


def results_of(logits, inv_label_map, slots=None, temperature=None, min_confidence=None, tuples=None, decode="independent"):
    """The result dictionaries of the callers' device route: ``results_from_slot_logits`` when a slot layout is given,
    ``results_from_logits`` otherwise; ``temperature`` is the callers' T (under slots: one, or one per slot); ``tuples`` /
    ``decode`` are ``results_from_slot_logits``' ``table`` / ``decode``."""
    check_decode(decode, tuples, slots is not None)
    if slots is not None:
        return results_from_slot_logits(logits, slots, inv_temperature=slot_inv_temperature_of(temperature, slots.n_slots),
                                        min_confidence=min_confidence, table=tuples, decode=decode)
    return results_from_logits(logits, inv_label_map, inv_temperature=inv_temperature_of(temperature), min_confidence=min_confidence)


def check_prototypes(prototypes, min_similarity, slots=None, temperature=None, min_confidence=None):
    """The callers' ``prototypes=`` / ``min_similarity=`` keywords: the prototype head replaces the ``fc`` head, so it goes with
    neither a slot layout nor that head's ``temperature`` / ``min_confidence``, and ``min_similarity`` needs a bank.  A
    caller's mistake is raised before any device call."""
    if prototypes is None:
        if min_similarity is not None:
            raise ValueError("min_similarity= needs prototypes= (a sir_amd.prototypes.PrototypeBank)")
        return
    if slots is not None:
        raise ValueError("prototypes= and slots= are two different heads: pass one of them")
    if temperature is not None or min_confidence is not None:
        raise ValueError("temperature= and min_confidence= belong to the fc head: with prototypes= use the bank's scale and "
                         "min_similarity=")
    if min_similarity is not None:
        float(min_similarity)


def results_from_prototypes(emb, bank, k=3, scale=None, min_similarity=None):
    """``results_from_logits`` for the prototype head: ONE ``sir_proto_score`` launch and ONE device-to-host copy for all rows of
    ``emb`` [B, 512] (``CNNAudioGRU.embed``) against ``bank`` (``sir_amd.prototypes.PrototypeBank``) -> list of B dicts of
    ``results_from_logits``' shape (labels are the bank's names; ``top_predictions`` holds at most as many entries as classes
    have a prototype) plus ``"similarity"`` (the rank-0 cosine) and ``"nearest"`` (the prototype row it belongs to).  With
    ``min_similarity`` set every dict also carries ``"rejected"``: the similarity is below it (or NaN)."""
    k = int(k)
    s = bank.score(emb, k=k, scale=scale)
    idx_h, near_h, prob_h, sim_h = _to_host(s.classes, s.nearest[:, None], s.probs, s.sims)
    names = bank.names
    results = []
    for row_i, near, row_p, row_s in zip(idx_h.tolist(), near_h[:, 0].tolist(), prob_h.tolist(), sim_h.tolist()):
        top = [{"label": names[i] if 0 <= i < len(names) else "Unknown", "probability": p}
               for i, p in zip(row_i, row_p) if not (i < 0 and p == 0.0)]              # (-1 / 0: a rank that does not exist)
        res = {"predicted_label": names[row_i[0]] if 0 <= row_i[0] < len(names) else "Unknown", "confidence": row_p[0],
               "top_predictions": top, "similarity": row_s[0], "nearest": near}
        if min_similarity is not None:
            res["rejected"] = _rejected(row_s[0], min_similarity)
        results.append(res)
    return results


def results_from_logits(logits, inv_label_map, k=3, inv_temperature=None, min_confidence=None):
    """``test_model._result`` for a whole batch: ONE ``sir_classify`` launch and ONE device-to-host copy for all rows of
    ``logits`` [B, C] -> list of B dicts of ``_result``'s shape (``top_predictions`` holds ``k`` entries, at most the number of
    classes; ``k`` above 8 is refused by ``ops.classify``).  ``inv_temperature`` (None, a number or
    ``metrics.fit_temperature``'s device scalar) calibrates the probabilities; with ``min_confidence`` set every dict also carries ``"rejected"``: the confidence is below it (or NaN)."""
    k = min(int(k), int(logits.shape[1]))
    idx, prob = ops.classify(logits, k=k, inv_temperature=inv_temperature)
    idx_h, prob_h = _to_host(idx, prob)
    results = []
    for row_i, row_p in zip(idx_h.tolist(), prob_h.tolist()):
        res = {"predicted_label": inv_label_map.get(row_i[0], "Unknown"), "confidence": row_p[0],
               "top_predictions": [{"label": inv_label_map.get(i, "Unknown"), "probability": p} for i, p in zip(row_i, row_p)]}
        if min_confidence is not None:
            res["rejected"] = _rejected(row_p[0], min_confidence)
        results.append(res)
    return results


@dataclasses.dataclass(frozen=True, eq=False)
class ResultOptions:
    """The result route of ``predict_frontend.predict_many``, ``IntentRecognizer.recognize_recordings`` and
    ``IntentRecognizer.open_streams``: their eight result keywords, checked once, and the one place that turns a model output
    into result dictionaries.  A wrong combination raises ``ValueError`` on construction, before any device call.

    ``on_device``: the dictionaries of a batch come from ``results_from_logits`` (one ``sir_classify`` launch and one copy
    instead of several host round trips per row); without it every row goes through ``test_model._result``.
    ``temperature`` (T; probabilities of ``softmax(logits / T)``) and ``min_confidence`` (every dictionary also carries
    ``"rejected"``) belong to the device route: without ``on_device=True`` they are refused.
    ``slots`` (a ``sir_amd.slots.SlotSpec``; implies the device route): the logit row is read as slot heads and every result
    is ``results_from_slot_logits``' dictionary -- decoded slots, joint ``"confidence"``, per-slot tables; ``temperature`` may
    then hold one T per slot and ``min_confidence`` rejects on the joint value.
    ``decode="joint"`` (with ``tuples``, a ``slots.TupleTable``: only the tuples that exist) ranks whole label tuples
    instead: the slots of the best tuple, its probability as ``"confidence"``, the k best tuples, ``"valid_mass"`` under a
    table, as ``results_from_slot_logits`` describes.  Both need ``slots``.
    ``prototypes`` (a ``sir_amd.prototypes.PrototypeBank``; implies the device route): the prototype head instead of the
    ``fc`` head -- the model is asked for embeddings (``embed`` is true) and every result is ``results_from_prototypes``'
    dictionary, labels from the bank's names, ``"similarity"`` and ``"nearest"`` added; ``min_similarity`` adds ``"rejected"``
    by distance and needs a bank.  ``prototypes`` with ``slots`` (or with ``temperature`` / ``min_confidence``) is refused.

    After construction ``on_device`` is the resolved route (true under ``slots`` or ``prototypes``)."""
    on_device: bool = False
    temperature: object = None
    min_confidence: object = None
    slots: object = None
    tuples: object = None
    decode: str = "independent"
    prototypes: object = None
    min_similarity: object = None

    def __post_init__(self):
        check_prototypes(self.prototypes, self.min_similarity, self.slots, self.temperature, self.min_confidence)
        object.__setattr__(self, "on_device", bool(self.on_device or self.slots is not None or self.prototypes is not None))
        check_route(self.on_device, self.temperature, self.min_confidence)
        check_decode(self.decode, self.tuples, self.slots is not None)
        if self.slots is not None:
            slot_inv_temperature_of(self.temperature, self.slots.n_slots)

    @property
    def embed(self):
        """The model is to return embeddings (``model.embed``) instead of logits."""
        return self.prototypes is not None

    def results(self, output, inv_label_map):
        """``output`` (logits [B, C], or embeddings [B, 512] under ``embed``) -> list of B result dictionaries; none, and no
        library call, for an output of zero rows."""
        if output.shape[0] == 0:
            return []
        if self.prototypes is not None:
            return results_from_prototypes(output, self.prototypes, min_similarity=self.min_similarity)
        if self.on_device:
            return results_of(output, inv_label_map, self.slots, self.temperature, self.min_confidence, self.tuples, self.decode)
        from sir_amd.scripts import test_model                                 # (imported here: it loads the model code)
        return [test_model._result(output[row:row + 1], inv_label_map) for row in range(output.shape[0])]
