"""``CNNAudioGRU`` with the reference's constructor, ``forward`` signature and ``state_dict`` keys
(/root/reference/models/models.py:5-68), computed by hand-written HIP kernels on MI355X.

The sub-modules below exist only to own parameters/buffers under the reference's names
(``conv{1,2,3}.weight``, ``bn{1,2,3}.*``, ``gru.weight_ih_l0`` ..., ``attention.*``, ``fc.*``) and
to reproduce PyTorch's default initialisation; their own ``forward`` methods are never called.
``forward`` hands the pointers to ``sir_model_infer`` (eval) or to the fused training step
(train).  There is no CPU path: inputs must live on a HIP device.
"""
import torch
from torch import nn

from sir_amd import _native, ops

CONV_CHANNELS = (32, 64, 128)
GRU_HIDDEN = 256
N_MELS = 64


class CNNAudioGRU(nn.Module):
    def __init__(self, num_classes, input_channels=1):
        super().__init__()
        if input_channels != 1:
            raise ValueError("the HIP path is built for input_channels=1 (log-mel input)")
        cin = input_channels
        for i, cout in enumerate(CONV_CHANNELS, start=1):
            setattr(self, f"conv{i}", nn.Conv2d(cin, cout, kernel_size=3, stride=1, padding=1, bias=False))
            setattr(self, f"bn{i}", nn.BatchNorm2d(cout))
            cin = cout
        # kept for attribute compatibility (models.py:18-20); pooling/activation are fused in the kernels
        self.relu = nn.ReLU(inplace=True)
        self.pool = nn.MaxPool2d(2)
        self.dropout = nn.Dropout(0.5)          # defined but unused by the reference forward
        self.gru_input_size = CONV_CHANNELS[-1] * (N_MELS // 8)
        self.gru = nn.GRU(input_size=self.gru_input_size, hidden_size=GRU_HIDDEN, num_layers=2,
                          batch_first=True, bidirectional=True, dropout=0.5)
        self.attention = nn.Linear(2 * GRU_HIDDEN, 1)
        self.fc = nn.Linear(2 * GRU_HIDDEN, num_classes)
        self._ws = ops.Workspace()
        self._sir_wcache = None
        self._sir_token = ops.new_model_token()

    def _apply(self, fn, *args, **kwargs):
        self._sir_wcache = None             # .to()/.cuda()/.float() may move the storage
        self._sir_token = ops.new_model_token()
        return super()._apply(fn, *args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self._sir_wcache = None             # assign=True swaps the tensors themselves
        self._sir_token = ops.new_model_token()
        return out

    def __getstate__(self):
        """``copy.deepcopy`` and pickling take the module without what belongs to THIS object: the pointer struct (ctypes
        pointers cannot be copied, and would point at this object's tensors), the training step's gradient buffer and both
        workspaces.  ``__setstate__`` gives the copy a workspace and a token of its own."""
        state = self.__dict__.copy()
        for k in ("_sir_wcache", "_sir_wsrc", "_sir_wptrs", "_sir_train", "_ws", "_sir_token"):
            state.pop(k, None)
        return state

    def __setstate__(self, state):
        super().__setstate__(state)
        self._ws = ops.Workspace()
        self._sir_wcache = None
        self._sir_token = ops.new_model_token()

    def weights_changed(self):
        """Tell the model that parameters or buffers were rewritten in place behind torch's back -- ``p.data.copy_(...)``,
        ``p.data.mul_(...)``, a write through a raw pointer: no version counter moves, so the next call would reuse weight
        layouts prepared from the old values.  (Replaced tensors and modules, in-place updates under ``torch.no_grad()``,
        ``load_state_dict``, ``.to()`` and this package's own optimizer need no such call.)"""
        ops.bump_weights_epoch()
        return self

    def train(self, mode=True):
        """``nn.Module.train`` plus one thing: BatchNorm blocks frozen by ``sir_amd.finetune.freeze(model, {"bn_stats"})``
        go back to ``eval()`` afterwards, so that the ``model.train()`` at the top of every epoch does not silently bring
        the batch statistics back.  Without such a freeze this is ``nn.Module.train`` exactly."""
        super().train(mode)
        if mode:
            for name in getattr(self, "_sir_frozen_modules", ()):
                getattr(self, name).eval()
        return self

    def forward(self, x, lengths=None):
        """x: [B, 64, T] or [B, 1, 64, T] float32 on the GPU -> logits [B, num_classes].

        ``lengths`` (int tensor or list, frames per clip): the un-padded function -- row b is what the model
        gives ``x[b:b+1, ..., :lengths[b]]`` on its own (scripts/test_tts_samples.py feeds each file that way), for a whole
        batch of mixed-length clips in one launch sequence.  On the differentiable path it needs bn1, bn2 and bn3 in ``eval()``
        (``finetune.freeze(model, {"bn_stats"})``): logits and gradients are then those of the un-padded function
        (``sir_model_train_fwd_ragged`` / ``sir_model_train_bwd_emb`` with ``frames``; ``x.grad`` is zero at columns
        ``>= lengths[b]``).  With live batch statistics a clip has no result of its own, and ``SirError`` is raised.

        ``self.training and torch.is_grad_enabled()`` selects the differentiable path, as before; ``model.eval()`` keeps
        calling ``sir_model_infer``.  The differentiable path is differentiable with respect to the 29 parameters and, if
        ``x.requires_grad``, with respect to ``x``: ``x.grad`` has the shape of ``x`` (``dfeats`` of ``sir_model_train_bwd_emb``;
        rank-local under data parallelism; a double backward raises).  For the input gradient of a model in ``eval()`` mode -- saliency, FGSM --
        see ``sir_amd.explain``.  Inside the differentiable path the sub-modules are consulted the way torch consults
        them: ``bnK.training == False`` uses (and keeps) that block's running statistics, ``gru.training == False`` turns the
        inter-layer dropout off, and parameters with ``requires_grad == False`` receive no gradient and cost no backward
        work where it can be skipped.  With every sub-module in training mode and every parameter trainable nothing changes.

        The differentiable path is an ordinary ``torch.autograd.Function`` node, and any number of them may be live per model:
        ``(ce(model(x1), y1) + ce(model(x2), y2)).backward()``, backwards in any order, ``explain`` / ``forward_craft`` /
        ``predict`` between a forward and its backward -- every node keeps a training workspace of its own until the end of its
        backward (``sir_amd.leases``).  With ``retain_graph=True`` a second backward works while no other forward has run on this
        model since the first; after one it raises ``RuntimeError`` (its workspace went back to the model and was reused).
        ``RuntimeError`` too: ``x`` changed in place before the backward, or a parameter changed between a node's forward and
        its backward (an optimizer step -- ``FusedAdam.step()`` counts process-wide --, an in-place update,
        ``weights_changed()``)."""
        if self.training and torch.is_grad_enabled():
            from sir_amd import train_ops
            return train_ops.forward_train(self, x, lengths=lengths)
        return ops.model_infer(self, x, self._ws, lengths=lengths)

    @torch.no_grad()
    def predict(self, x, lengths=None):
        """logits and argmax (scripts/evaluate.py:82-83) in one launch sequence; ``lengths`` as in ``forward``."""
        return ops.model_infer(self, x, self._ws, want_argmax=True, lengths=lengths)

    @torch.no_grad()
    def embed(self, x, lengths=None):
        """The utterance embeddings [B, 512]: the attention-pooled context the classifier reads, raw (``ops.model_embed``);
        the classifier itself is not run.  ``lengths`` as in ``forward``.  ``sir_amd.prototypes.PrototypeBank`` enrols and
        scores these rows."""
        return ops.model_embed(self, x, self._ws, lengths=lengths)

    def forward_with_embedding(self, x, lengths=None):
        """``(logits [B, num_classes], emb [B, 512])`` in one pass, dispatched as ``forward`` is.  On the differentiable path
        (``self.training and torch.is_grad_enabled()``) both carry a graph (``train_ops.forward_train_embed``): a loss on ``emb``
        -- ``sir_amd.prototypes.ProxyHead`` -- trains the embedding that ``PrototypeBank`` enrols from, alone or beside the
        cross-entropy on ``logits``.  Otherwise the two are ``model(x)``'s logits and ``embed``'s rows, bit for bit."""
        if self.training and torch.is_grad_enabled():
            from sir_amd import train_ops
            return train_ops.forward_train_embed(self, x, lengths=lengths)
        with torch.no_grad():
            emb, logits, _ = ops.model_embed(self, x, self._ws, lengths=lengths, want_logits=True)
        return logits, emb

    @torch.no_grad()
    def classify(self, x, lengths=None, k=3, inv_temperature=None):
        """The forward plus ``ops.classify`` on the device -> ``(logits [B, C], topk_idx int32 [B, k], topk_prob [B, k])``: the
        ``k`` most probable classes of every clip in order and their softmax probabilities (``topk_idx[:, 0]`` is ``predict``'s
        argmax).  ``lengths`` as in ``forward`` (the ragged route), ``inv_temperature`` as in ``ops.classify``."""
        logits = ops.model_infer(self, x, self._ws, lengths=lengths)
        idx, prob = ops.classify(logits, k=k, inv_temperature=inv_temperature)
        return logits, idx, prob


if __name__ == "__main__":
    model = CNNAudioGRU(num_classes=31).cuda().eval()
    print("Output shape:", model(torch.randn(4, 64, 200, device="cuda")).shape)
