"""Inference pad skip (csrc/model_infer.hip): trailing all-+0.0 frame columns are not pushed through conv1-3 and the
layer-0 input projection; the GRU reads a template utterance's pre-activations there instead.  The results must be
bit-identical to the full path, which the same features with every +0.0 tail replaced by -0.0 force (non-zero bits)."""
import pytest
import torch

from oracle import model_ref
from sir_amd import ops, synth
from sir_amd.featurizer import get_featurizer
from sir_amd.models.models import CNNAudioGRU

pytestmark = pytest.mark.gpu
DEV = "cuda"
HOP = 512


@pytest.fixture(scope="module")
def sd():
    return synth.synth_state_dict(31, seed=0)


def _model(sd):
    m = CNNAudioGRU(31)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def _feats(lengths, t_pad, seed=5):
    """featurizer output for clips of the given sample lengths (0 = silence of 48 000 samples)"""
    n = len(lengths)
    lmax = max(max(lengths), 48000)
    wave = synth.synth_clips(n, lmax, seed=seed)
    lens = []
    for i, L in enumerate(lengths):
        if L == 0:
            wave[i] = 0.0
            L = 48000
        wave[i, L:] = 0.0
        lens.append(L)
    lt = torch.tensor(lens, dtype=torch.int32, device=DEV)
    t_all = max(t_pad, 1 + lmax // HOP)                               # clips longer than t_pad frames are cut, as the data loaders do
    return get_featurizer()(wave.to(DEV), lt, t_pad=t_all)[:, :, :t_pad].contiguous()


def _extent(x):
    """1 + last frame column with any bit set, per utterance"""
    nz = (x.view(torch.int32) != 0).any(dim=1)                       # [B, T]
    idx = torch.arange(x.shape[2], device=x.device) + 1
    return (nz * idx).amax(dim=1)


def _neg_tail(x):
    """the same features with the all-+0.0 tail of every utterance replaced by -0.0 (forces the full path)"""
    e = _extent(x)
    cols = torch.arange(x.shape[2], device=x.device)
    tail = (cols[None, None, :] >= e[:, None, None]).expand_as(x)
    return torch.where(tail, torch.full_like(x, -0.0), x)


def _infer(m, x, ws=None):
    ws = ws if ws is not None else ops.Workspace()
    logits, amax = ops.model_infer(m, x, ws, want_argmax=True)
    torch.cuda.synchronize()
    return logits, amax


MIXED = [700, 8000, 16000, 32000, 48000, 47999, 0, 144000]


@pytest.mark.parametrize("bsz,t_pad", [(1, 200), (5, 37), (256, 200)])
def test_skip_equals_full_path(sd, bsz, t_pad):
    m = _model(sd)
    lengths = [MIXED[i % len(MIXED)] for i in range(bsz)]
    x = _feats(lengths, t_pad)
    xf = _neg_tail(x)
    assert not torch.equal(x.view(torch.int32), xf.view(torch.int32)) or bool((_extent(x) == t_pad).all())
    lg, am = _infer(m, x)
    lgf, amf = _infer(m, xf)
    assert torch.equal(lg, lgf)
    assert torch.equal(am, amf)


def test_no_tail_94_frames(sd):
    m = _model(sd)
    x = _feats([48000] * 8, 94)
    assert bool((_extent(x) == 94).all())
    lg, am = _infer(m, x)
    with torch.no_grad():
        ref = model_ref.forward(sd, x.cpu())
    assert (lg.cpu() - ref).abs().max().item() <= 2e-4
    assert torch.equal(am.cpu(), ref.argmax(1))


def test_mixed_batch_oracle(sd):
    m = _model(sd)
    x = _feats(MIXED * 2, 200)
    lg, am = _infer(m, x)
    with torch.no_grad():
        ref = model_ref.forward(sd, x.cpu())
    assert (lg.cpu() - ref).abs().max().item() <= 2e-4
    assert torch.equal(am.cpu(), ref.argmax(1))


def test_skip_leaves_pad_columns_unwritten(sd):
    m = _model(sd)
    x = _feats([48000] * 16, 200)                                     # 94 frames: E0 = 94, GRU steps 0..12 see data
    assert bool((_extent(x) == 94).all())
    need = ops._native.lib().sir_model_workspace_bytes(get_featurizer().handle, 16, 200, 0)
    ws = ops.Workspace()
    ws.get(need, x.device).fill_(0xFF)                                # NaN bit pattern everywhere
    dbg = {}
    lg = ops.model_infer(m, x, ws, debug=dbg)
    torch.cuda.synchronize()
    c1 = dbg["conv1"].view(torch.int32)                               # [B, 32, 100, 32] NHWC
    c2 = dbg["conv2"].view(torch.int32)                               # [B, 16, 50, 64]
    # conv1: pooled columns 0..54 demanded, stored exactly; conv2: 27 demanded, computed in 4-column tasks (28)
    assert bool((c1[:, :, 55:, :] == -1).all())
    assert bool((c2[:, :, 28:, :] == -1).all())
    dbg_full = {}
    lgf = ops.model_infer(m, _neg_tail(x), ops.Workspace(), debug=dbg_full)
    torch.cuda.synchronize()
    assert torch.equal(dbg["conv1"][:, :, :55].view(torch.int32), dbg_full["conv1"][:, :, :55].view(torch.int32))
    assert torch.equal(dbg["conv2"][:, :, :27].view(torch.int32), dbg_full["conv2"][:, :, :27].view(torch.int32))
    assert torch.equal(dbg["gru_in"][:, :13].view(torch.int32), dbg_full["gru_in"][:, :13].view(torch.int32))
    assert torch.equal(lg, lgf)


def test_permuted_batch(sd):
    m = _model(sd)
    x = _feats(MIXED * 4, 200)
    perm = torch.randperm(x.shape[0], generator=torch.Generator().manual_seed(3)).to(DEV)
    lg, _ = _infer(m, x)
    lgp, _ = _infer(m, x[perm].contiguous())
    assert torch.equal(lg[perm], lgp)


def test_nan_in_tail(sd):
    m = _model(sd)
    x = _feats([48000] * 4 + [16000] * 4, 200)
    x[1, 7, 150] = float("nan")
    x[5, 0, 120] = float("nan")
    lg, am = _infer(m, x)
    lgf, amf = _infer(m, _neg_tail(x))
    assert torch.equal(lg.isnan(), lgf.isnan())
    assert torch.equal(torch.nan_to_num(lg), torch.nan_to_num(lgf))
    assert torch.equal(am, amf)
    # the NaN is data on both paths: its rows are NaN throughout (include/sir_hip.h at sir_model_infer), the others untouched
    assert lg[[1, 5]].isnan().all() and not lg[[0, 2, 3, 4, 6, 7]].isnan().any()


@pytest.mark.parametrize("n_streams", [2, 3])
def test_pipeline_streams(sd, n_streams):
    from sir_amd.pipeline import BatchPipeline
    m = _model(sd)
    batches = [_feats([MIXED[(i + j) % len(MIXED)] for j in range(32)], 200, seed=11 + i) for i in range(5)]
    ref = [_infer(m, b)[0] for b in batches]
    pipe = BatchPipeline(m, n_streams=n_streams)
    outs = [pipe.infer(i, b)[0] for i, b in enumerate(batches)]
    pipe.synchronize()
    for a, b in zip(outs, ref):
        assert torch.equal(a, b)
