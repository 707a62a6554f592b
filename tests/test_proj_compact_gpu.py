"""Layer-0 input projection over a row list (csrc/model_infer.hip, infer_tables.h, f16x3_kernels.h): with the pad skip on, the projection
computes only the rows the layer-0 recurrence reads (steps s < d3 of every utterance and the template utterance's S rows), on
a 96-, 128- or 160-row tile chosen on the device from the real row count.  Every output element keeps the dense kernel's MFMA
sequence, so logits stay bit-identical to the full path, which the same features with -0.0 tails force.  The workspace starts
as 0xFF (NaN bits): a listed row left unwritten would surface as NaN."""
import pytest
import torch

from sir_amd import ops, synth
from sir_amd.featurizer import get_featurizer
from sir_amd.models.models import CNNAudioGRU

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def model():
    m = CNNAudioGRU(31)
    m.load_state_dict(synth.synth_state_dict(31, seed=0))
    return m.to(DEV).eval()


def _feats_d3(d3, t=200, seed=0):
    """random features [B, 64, t] whose data extent gives each utterance exactly d3[u] GRU steps that see data
    (d3 = min(S, (E0 + 14) // 8), E0 = 1 + last column with any bit set); the tails are +0.0"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(len(d3), 64, t, generator=g) + 3.0                 # no exact zeros inside the data
    for u, d in enumerate(d3):
        e0 = min(t, max(1, 8 * d - 14))
        assert min(t // 8, (e0 + 14) // 8) == d
        x[u, :, e0:] = 0.0
    return x.to(DEV)


def _neg_tail(x):
    nz = (x.view(torch.int32) != 0).any(dim=1)
    e0 = (nz * (torch.arange(x.shape[2], device=x.device) + 1)).amax(dim=1)
    tail = (torch.arange(x.shape[2], device=x.device)[None, None, :] >= e0[:, None, None]).expand_as(x)
    return torch.where(tail, torch.full_like(x, -0.0), x)


def _tile(count, ncu, n_tiles=6):
    """the tile the row-list kernel picks: the smallest whose workgroups fit one per CU, else 160 rows"""
    for bm in (96, 128):
        if -(-count // bm) * n_tiles <= ncu:
            return bm
    return 160


def _check(model, d3, t=200, seed=0):
    x = _feats_d3(d3, t, seed)
    bsz = x.shape[0]
    ws = ops.Workspace()
    ws.get(ops._native.lib().sir_model_workspace_bytes(get_featurizer().handle, bsz, t, 0), x.device).fill_(0xFF)
    lg, am = ops.model_infer(model, x, ws, want_argmax=True)
    lgf, amf = ops.model_infer(model, _neg_tail(x), ops.Workspace(), want_argmax=True)
    torch.cuda.synchronize()
    tabs, s = ops.pad_skip_tables(ws.buf, bsz, t), t // 8
    d3w, rows = tabs["d3"], tabs["rows"]
    want = [u * s + k for u in range(bsz + 1) for k in range(int(d3w[u]))]
    assert d3w[:bsz].tolist() == list(d3) and int(d3w[bsz]) == s
    assert rows.tolist() == want
    assert not lg.isnan().any()
    assert torch.equal(lg.view(torch.int32), lgf.view(torch.int32))
    assert torch.equal(am, amf)
    return len(want)


@pytest.mark.parametrize("bsz", [1, 5, 16, 256])
def test_mixed_lengths(model, bsz):
    g = torch.Generator().manual_seed(bsz)
    d3 = torch.randint(1, 26, (bsz,), generator=g).tolist()
    d3[0] = 13                                                        # the bench clip: 94 of 200 frames
    _check(model, d3, seed=bsz)


def test_short_clips_odd_frames(model):
    _check(model, [1, 2, 3, 4, 1], t=37)


def test_batch_beyond_one_utterance_per_thread(model):
    """more than 1023 utterances: pad_tables_kernel's threads take several utterances each"""
    _check(model, [1 + (u * 7) % 4 for u in range(1100)], t=37)


def test_no_padding_keeps_160_row_tile(model):
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    count = _check(model, [25] * 256)
    assert count == 257 * 25
    assert _tile(count, ncu) == 160


@pytest.mark.parametrize("bm", [96, 128])
def test_tile_switch_boundaries(model, bm):
    """row counts on each side of the largest count the bm-row tile takes: bm rows there, a larger tile one row later"""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    bsz, s = 256, 25
    edge = ncu // 6 * bm                                              # largest row count whose bm-row tiles fit one per CU
    if not bsz + s <= edge - s <= bsz * s - 1:
        pytest.skip(f"{ncu} CUs: the {bm}-row edge lies outside what a batch of {bsz} can reach")
    for count in (edge, edge + 1):
        total = count - s                                             # sum of d3 over the real utterances
        base, extra = divmod(total, bsz)
        d3 = [base + 1] * extra + [base] * (bsz - extra)
        assert _check(model, d3, seed=count) == count
    assert _tile(edge, ncu) == bm and _tile(edge + 1, ncu) > bm


def test_published_tables_d1_rows_nonfinite(model):
    """the tables ops.pad_skip_tables reads through sir_model_infer_table_offsets, after a padded call: conv1 columns d1 from d3
    (formulas at the head of csrc/infer_tables.h; the template at full width), the row list with the template's rows last, and the
    non-finite flags -- one inf inside utterance 1's data"""
    t, d3 = 24, [3, 1, 2]
    bsz, s, wp1, wp2 = len(d3), t // 8, t // 2, t // 4
    x = _feats_d3(d3, t)
    x[1, 5, 0] = float("inf")
    ws = ops.Workspace()
    ws.get(ops._native.lib().sir_model_workspace_bytes(get_featurizer().handle, bsz, t, 0), x.device).fill_(0xFF)
    ops.model_infer(model, x, ws)
    torch.cuda.synchronize()
    tabs = ops.pad_skip_tables(ws.buf, bsz, t)
    assert tabs["d3"].tolist() == d3 + [s]
    assert tabs["d1"].tolist() == [min(wp1, 2 * min(wp2, 2 * d + 1) + 1) for d in d3] + [wp1]
    assert tabs["rows"].tolist() == [u * s + k for u, d in enumerate(d3 + [s]) for k in range(d)]
    assert tabs["nonfinite"].tolist() == [0, 1, 0]
