"""What tests/test_weight_mutation_gpu.py and tests/test_weight_mutation_host.py share: the seeded mutations of single
tensors and the routes by which a model's tensors can be REPLACED between two calls (not a test module).

Every mutation is one float32 operation on values both sides hold exactly (``t + delta``, ``t * factor``), so the state dict
the oracle gets and the tensors on the device agree bit for bit.  Magnitudes: ``0.5 * std * randn`` added to a tensor moves
the oracle's logits on ``X`` by at least 5e-3 for every tensor but two; ``attention.weight`` needs ``2 * std * randn`` (0.5 moves
them by 4e-4 only) and ``attention.bias`` cannot move them at all (softmax is shift-invariant): it is left out.
``running_var`` is multiplied by ``1 + 0.5 * rand`` so that it stays positive."""
import zlib

import torch
from torch import nn

from sir_amd import synth

NUM_CLASSES = 31
NEW_CLASSES = 6
FLOOR = 1e-3            # every mutation must move the ORACLE's logits by at least this: 50 x the parity bound
TOL = 2e-5              # |logits - oracle|, the bound of test_model_gpu.py::test_odd_batch_and_short_input
LENGTHS = [64, 40, 9]


def base_state_dict():
    return synth.synth_state_dict(NUM_CLASSES, seed=0)


def features(seed=21):
    return synth.synth_features(3, 64, seed=seed)


def float_keys(sd):
    """the float parameters and buffers whose value the logits depend on (``num_batches_tracked`` is an integer)"""
    return [k for k, v in sd.items() if v.is_floating_point() and k != "attention.bias"]


def delta(key, t):
    """``(op, operand)``: the seeded mutation of tensor ``key`` with the current value ``t`` (CPU float32)"""
    g = torch.Generator().manual_seed(zlib.crc32(key.encode()))
    if key.endswith("running_var"):
        return "mul", 1.0 + 0.5 * torch.rand(t.shape, generator=g)
    scale = 2.0 if key == "attention.weight" else 0.5
    return "add", scale * float(t.std()) * torch.randn(t.shape, generator=g)


def mutated(key, t):
    """the mutated value of ``t`` on the CPU, out of place"""
    op, d = delta(key, t)
    return t * d if op == "mul" else t + d


def mutate_(t, key, value):
    """the same mutation in place on ``t`` (any device; ``value``: the tensor's current value on the CPU)"""
    op, d = delta(key, value)
    d = d.to(t.device)
    return t.mul_(d) if op == "mul" else t.add_(d)


def tensor_of(model, key):
    obj = model
    for part in key.split("."):
        obj = getattr(obj, part)
    return obj


def cpu_state(model):
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}


# ---- routes that replace tensors or modules (sections 1b / 1c of the weight-mutation tests) -------------------------------
def _new(model, key, dev):
    return mutated(key, tensor_of(model, key).detach().cpu()).to(dev)


def swap_head(model, dev, num_classes=NEW_CLASSES):
    head = synth.synth_state_dict(num_classes, seed=3)
    fc = nn.Linear(512, num_classes)
    with torch.no_grad():
        fc.weight.copy_(head["fc.weight"])
        fc.bias.copy_(head["fc.bias"])
    model.fc = fc.to(dev)


def assign_parameter(key):
    def route(model, dev):
        owner, _, leaf = key.rpartition(".")
        setattr(tensor_of(model, owner), leaf, nn.Parameter(_new(model, key, dev)))
    return route


def assign_data(model, dev):
    for key in ("conv2.weight", "gru.weight_hh_l0_reverse", "fc.bias", "bn3.running_mean"):
        tensor_of(model, key).data = _new(model, key, dev)


def vector_to_parameters(model, dev):
    new = {key: _new(model, key, dev) for key in ("conv2.weight", "gru.weight_ih_l1", "fc.weight")}
    vec = torch.cat([new.get(k, p.detach()).reshape(-1) for k, p in model.named_parameters()])
    nn.utils.vector_to_parameters(vec, model.parameters())


def child_round_trip(name, key):
    """the child's own ``_apply`` (``model.gru.cpu()`` ... ``model.gru.to(dev)``; for a CPU model, where ``.cpu()`` moves nothing,
    ``.double()`` ... ``.float()``), with ``key`` edited while the child is away"""
    def route(model, dev):
        child = getattr(model, name)
        value = tensor_of(model, key).detach().cpu().float()
        if torch.device(dev).type == "cpu":
            child.double()
        else:
            child.cpu()
        with torch.no_grad():
            tensor_of(model, key).copy_(mutated(key, value))
        child.to(dev).float()
    return route


def load_assign(model, dev):
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    for key in ("conv3.weight", "attention.weight"):
        sd[key] = _new(model, key, dev)
    model.load_state_dict(sd, assign=True)


ROUTES = {
    "head_swap": swap_head,
    "parameter_assign_prepared": assign_parameter("conv3.weight"),
    "parameter_assign_direct": assign_parameter("gru.bias_ih_l1"),
    "data_assign": assign_data,
    "vector_to_parameters": vector_to_parameters,
    "child_round_trip_gru": child_round_trip("gru", "gru.weight_ih_l0"),
    "child_round_trip_bn2": child_round_trip("bn2", "bn2.running_var"),
    "load_state_dict_assign": load_assign,
}
