"""Inference conv1's launch grid (csrc/model_kernels.h, conv1_mfma_bn_relu_pool_body): the utterance is the fastest-varying part of
the workgroup id, the 32-column strip the slowest.  Only the decoding of (utterance, strip) changed, so every stored
bit must be what it was -- checked the way tests/test_pad_skip_gpu.py does: the same features with every +0.0 tail replaced by -0.0
force the full path, and the debug dictionary of ops.model_infer returns the conv1 map.  The cases sit where an index remap can go
wrong: utterances with 1 to 4 live strips side by side, batch sizes for which B + 1 (the template utterance is the last id of each
strip) is a multiple of neither 8 nor the strip count, widths that are no multiple of the strip, a permuted batch, and the ragged
call (which takes its utterance count from the grid).  Everything here is bit-equality: no tolerance."""
import pytest
import torch

import cases
from sir_amd import _native, ops, synth
from sir_amd.featurizer import get_featurizer
from sir_amd.models.models import CNNAudioGRU

pytestmark = pytest.mark.gpu
DEV = "cuda"
HOP = 512
LENGTHS = [0, 700, 16000, 32000, 48000, 70000, 144000]               # samples; 0 = silence
D1_AT_200 = [7, 11, 23, 39, 55, 75, 100]                              # conv1 columns these demand at t_pad = 200
STRIPS_AT_200 = [1, 1, 1, 2, 2, 3, 4]                                 # live 32-column strips


@pytest.fixture(scope="module")
def model():
    m = CNNAudioGRU(31)
    m.load_state_dict(synth.synth_state_dict(31, seed=0))
    return m.to(DEV).eval()


def _feats(lengths, t_pad, seed=5):
    """featurizer output for clips of the given sample lengths (0 = silence), padded or cut to t_pad frames"""
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
    t_all = max(t_pad, 1 + lmax // HOP)
    return get_featurizer()(wave.to(DEV), lt, t_pad=t_all)[:, :, :t_pad].contiguous()


def _extent(x):
    """1 + last frame column with any bit set, per utterance"""
    nz = (x.view(torch.int32) != 0).any(dim=1)
    idx = torch.arange(x.shape[2], device=x.device) + 1
    return (nz * idx).amax(dim=1)


def _neg_tail(x):
    """the same features with the all-+0.0 tail of every utterance replaced by -0.0 (forces the full path)"""
    e = _extent(x)
    cols = torch.arange(x.shape[2], device=x.device)
    tail = (cols[None, None, :] >= e[:, None, None]).expand_as(x)
    return torch.where(tail, torch.full_like(x, -0.0), x)


def _d1(e0, t_pad):
    """conv1 columns an utterance of extent e0 demands: the formulas at the head of csrc/infer_tables.h, on the host"""
    wp1, wp2 = t_pad // 2, t_pad // 4
    s = wp2 // 2
    d3 = min(s, (e0 + 14) // 8)
    d2 = min(wp2, 2 * d3 + 1)
    return min(wp1, 2 * d2 + 1)


def _filled_ws(bsz, t_pad):
    need = _native.lib().sir_model_workspace_bytes(get_featurizer().handle, bsz, t_pad, 0)
    ws = ops.Workspace()
    ws.get(need, torch.device(DEV)).fill_(0xFF)                       # -1 as int32, a NaN as float32
    return ws


def _compare_with_full_path(model, lengths, t_pad):
    """pad-skip call on a 0xFF-filled workspace against the full path -> the expected d1 per utterance"""
    x = _feats(lengths, t_pad)
    e0 = _extent(x).tolist()
    for L, e in zip(lengths, e0):                                     # frames of a centred STFT; silence has no bit set
        assert e == (0 if L == 0 else min(t_pad, 1 + L // HOP)), (L, e)
    d1 = [_d1(e, t_pad) for e in e0]
    dbg, dbg_full = {}, {}
    lg, am = ops.model_infer(model, x, _filled_ws(len(lengths), t_pad), want_argmax=True, debug=dbg)
    lgf, amf = ops.model_infer(model, _neg_tail(x), ops.Workspace(), want_argmax=True, debug=dbg_full)
    torch.cuda.synchronize()
    c1, c1f = dbg["conv1"].view(torch.int32), dbg_full["conv1"].view(torch.int32)    # [B, 32, wp1, 32] NHWC
    assert c1.shape[2] == t_pad // 2
    for b, d in enumerate(d1):
        assert torch.equal(c1[b, :, :d], c1f[b, :, :d]), (b, d)
        assert bool((c1[b, :, d:] == -1).all()), (b, d)
    assert not bool((c1f == -1).any())                                # (a NaN the full path stores would be 0x7FC00000)
    assert torch.equal(lg.view(torch.int32), lgf.view(torch.int32))
    assert torch.equal(am, amf)
    ops.check_status()
    return d1


@pytest.mark.parametrize("bsz", [1, 7, 9])
def test_mixed_live_strips(model, bsz):
    """utterances with 1, 1, 1, 2, 2, 3 and 4 live strips of 4 side by side (batch 1: the 2-strip one)"""
    pick = [(i + 4) % len(LENGTHS) for i in range(bsz)]
    d1 = _compare_with_full_path(model, [LENGTHS[i] for i in pick], 200)
    assert d1 == [D1_AT_200[i] for i in pick]
    assert [(d + 31) // 32 for d in d1] == [STRIPS_AT_200[i] for i in pick]


@pytest.mark.parametrize("t_pad,wp1,strips", [(136, 68, 3), (37, 18, 1)])
def test_width_not_a_multiple_of_the_strip(model, t_pad, wp1, strips):
    """wp1 = 68: three strips, the last with 4 columns; wp1 = 18: one partial strip"""
    assert t_pad // 2 == wp1 and (wp1 + 31) // 32 == strips and wp1 % 32 != 0
    d1 = _compare_with_full_path(model, [0, 16000, 48000, 70000, 144000], t_pad)
    assert max(d1) == wp1 and min(d1) < wp1


def test_permuted_batch(model):
    x = _feats([LENGTHS[i % len(LENGTHS)] for i in range(9)], 200)
    perm = torch.randperm(9, generator=torch.Generator().manual_seed(3)).to(DEV)
    lg = ops.model_infer(model, x, _filled_ws(9, 200))
    lgp = ops.model_infer(model, x[perm].contiguous(), _filled_ws(9, 200))
    torch.cuda.synchronize()
    assert torch.equal(lg[perm].view(torch.int32), lgp.view(torch.int32))


def _ragged(model, x, frames):
    """one ragged call (ops.model_infer(..., lengths=...), as tests/test_ragged_infer_gpu.py) on a NaN-filled workspace"""
    lengths = torch.tensor(frames, dtype=torch.int32, device=DEV)
    lg, am = ops.model_infer(model, x, _filled_ws(x.shape[0], x.shape[-1]), want_argmax=True, lengths=lengths)
    torch.cuda.synchronize()
    return lg.cpu(), am.cpu()


def test_ragged_clip_alone_and_in_a_batch(model):
    """9 clips whose conv1 widths frames / 2 = 4 ... 100 take 1, 1, 2, 2, 2, 3, 3, 4 and 4 strips: each clip alone in a batch of one
    gives the bits of its row in the batch (the ragged kernel reads the utterance count off the grid)"""
    frames = [8, 64, 66, 94, 128, 130, 192, 194, 200]
    assert [((f // 2) + 31) // 32 for f in frames] == [1, 1, 2, 2, 2, 3, 3, 4, 4]
    x = cases.varied_features(9, 200, seed=11).float()
    for b, f in enumerate(frames):
        x[b, :, f:] = float("nan")                                    # nothing behind a clip's length may be read
    x = x.to(DEV)
    lg, am = _ragged(model, x, frames)
    assert not lg.isnan().any()
    for b, f in enumerate(frames):
        lg1, am1 = _ragged(model, x[b:b + 1].contiguous(), [f])
        assert torch.equal(lg1.view(torch.int32), lg[b:b + 1].view(torch.int32)), (b, f)
        assert torch.equal(am1, am[b:b + 1]), (b, f)
    ops.check_status()
