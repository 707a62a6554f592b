"""Tile rule of the row-list input projection (csrc/f16x3_kernels.h, gemm_nt_f16x3_gather_kernel): a call from a handle whose
recurrence launches come from one stream takes the LATENCY rule (the smallest of 96 / 128 / 160 rows whose tiles fit one
workgroup per CU), a call from a handle in chained mode (launches alternating between streams, BatchPipeline with two slots) the
THROUGHPUT rule (the tile that holds the least CU time, above a floor of 96-row tiles).  Workgroup 0 records the row count it read
and the tile it chose behind the pad-skip tables (ops.proj_tile_record); both rules are mirrored here on the host.  Every tile
gives the same bits, so logits and argmax of the pipelined call equal the serial call's.  Workspaces start as 0xFF (NaN bits)."""
import pytest
import torch

from sir_amd import ops, synth
from sir_amd.featurizer import get_featurizer
from sir_amd.models.models import CNNAudioGRU
from sir_amd.pipeline import BatchPipeline

pytestmark = pytest.mark.gpu
DEV = "cuda"
T, S = 200, 25
# h3_gather_cost / H3_TP_FLOOR in csrc/f16x3_kernels.h (time of one tile on a CU of its own, 0.1 us; floor in 96-row tiles)
COST = {1024: {96: 402, 128: 447, 160: 513}, 512: {96: 236, 128: 261, 160: 294}}
TP_FLOOR = 108
N_TILES = 6                                                           # 2 directions x 768 / 256 column blocks per row tile
FLOOR_EDGE = TP_FLOOR // N_TILES * 96                                 # the largest row count the floor keeps on the latency rule
SETTLE = 34                                                           # serial calls (2 recurrence launches each) that end chained mode: 1 + 64 launches


@pytest.fixture(scope="module")
def model():
    m = CNNAudioGRU(31)
    m.load_state_dict(synth.synth_state_dict(31, seed=0))
    return m.to(DEV).eval()


def _feats_d3(d3, t=T, seed=0):
    """random features [B, 64, t] whose data extent gives each utterance exactly d3[u] GRU steps that see data
    (d3 = min(S, (E0 + 14) // 8), E0 = 1 + last column with any bit set); the tails are +0.0"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(len(d3), 64, t, generator=g) + 3.0                 # no exact zeros inside the data
    for u, d in enumerate(d3):
        e0 = min(t, max(1, 8 * d - 14))
        assert min(t // 8, (e0 + 14) // 8) == d
        x[u, :, e0:] = 0.0
    return x.to(DEV)


def _d3_for(count):
    """d3 of 3 .. 16 utterances (more above 425 rows) whose row list, sum(d3) + the template's S rows, has `count` rows"""
    total = count - S
    bsz = max(3, -(-total // 20))
    base, extra = divmod(total, bsz)
    d3 = [base + 1] * extra + [base] * (bsz - extra)
    assert 1 <= min(d3) and max(d3) <= S and sum(d3) + S == count
    return d3


def _latency(count, ncu):
    for bm in (96, 128):
        if -(-count // bm) * N_TILES <= ncu:
            return bm
    return 160


def _throughput(count, ncu, k=1024):
    if -(-count // 96) * N_TILES <= TP_FLOOR:
        return _latency(count, ncu)
    c = {bm: -(-count // bm) * COST[k][bm] for bm in (96, 128, 160)}
    return 96 if c[96] <= c[128] and c[96] <= c[160] else 128 if c[128] <= c[160] else 160


def _fresh_ws(x):
    ws = ops.Workspace()
    ws.get(ops._native.lib().sir_model_workspace_bytes(get_featurizer().handle, x.shape[0], x.shape[2], 0), x.device).fill_(0xFF)
    return ws


def _serial(model, x, lengths=None, calls=SETTLE):
    """`calls` calls on the current stream, enough to end a chained mode left by whoever used the handle before ->
    (logits, argmax, record) of the last one"""
    ws = _fresh_ws(x)
    for _ in range(calls):
        lg, am = ops.model_infer(model, x, ws, want_argmax=True, lengths=lengths)
    torch.cuda.synchronize()
    return lg, am, ops.proj_tile_record(ws.buf, x.shape[0], x.shape[2])


def _pipelined(model, x, lengths=None, batches=4):
    """the same batch `batches` times through two alternating slots -> per batch (logits, argmax, record), the last two"""
    pipe = BatchPipeline(model, n_streams=2)
    pipe.workspaces = [_fresh_ws(x) for _ in range(2)]
    torch.cuda.synchronize()
    out = []
    for i in range(batches):
        k = pipe.slot(i)
        lg, am = pipe.infer(i, x, want_argmax=True, lengths=lengths)
        out.append((k, lg, am))
    pipe.synchronize()
    return [(lg, am, ops.proj_tile_record(pipe.workspaces[k].buf, x.shape[0], x.shape[2])) for k, lg, am in out[-2:]]


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def test_rules_differ_above_the_floor_only():
    """the two mirrored rules on the counts below: equal up to the floor's edge, 160 against 96 rows one row later (256 CUs)"""
    assert _throughput(FLOOR_EDGE, 256) == _latency(FLOOR_EDGE, 256) == 96
    assert _throughput(FLOOR_EDGE + 1, 256) == 160 and _latency(FLOOR_EDGE + 1, 256) == 96
    assert _throughput(3353, 256) == 160 and _latency(3353, 256) == 96        # the bench shape: 126 workgroups against 210


@pytest.mark.parametrize("count", [96, 97, 160, 161, 192, 193, 320, 321, FLOOR_EDGE, FLOOR_EDGE + 1])
def test_serial_and_pipelined(model, count):
    ncu = _ncu()
    x = _feats_d3(_d3_for(count), seed=count)
    lg, am, rec = _serial(model, x)
    assert rec == (count, _latency(count, ncu))
    assert not lg.isnan().any()
    for lgp, amp, recp in _pipelined(model, x):
        assert recp == (count, _throughput(count, ncu))
        assert not lgp.isnan().any()
        assert torch.equal(lgp.view(torch.int32), lg.view(torch.int32))
        assert torch.equal(amp, am)


def test_ragged_pipelined(model):
    """ragged: no template rows; both projections run over the list and the record is layer 1's (K = 512)"""
    ncu = _ncu()
    for count, steps in ((97, [25, 25, 25, 20, 2]), (161, [25, 25, 25, 25, 25, 25, 10, 1])):
        assert sum(steps) == count
        g = torch.Generator().manual_seed(count)
        x = (torch.randn(len(steps), 64, T, generator=g) + 3.0).to(DEV)
        lengths = torch.tensor([8 * s for s in steps], dtype=torch.int32, device=DEV)
        lg, am, rec = _serial(model, x, lengths)
        assert rec == (count, _latency(count, ncu))
        assert not lg.isnan().any()
        for lgp, amp, recp in _pipelined(model, x, lengths):
            assert recp == (count, _throughput(count, ncu, 512))
            assert not lgp.isnan().any()
            assert torch.equal(lgp.view(torch.int32), lg.view(torch.int32))
            assert torch.equal(amp, am)


def test_falls_back_after_64_launches_from_one_stream(model):
    ncu = _ncu()
    count = FLOOR_EDGE + 1
    x = _feats_d3(_d3_for(count), seed=1)
    assert _throughput(count, ncu) != _latency(count, ncu)
    assert all(rec == (count, _throughput(count, ncu)) for _, _, rec in _pipelined(model, x))
    _, _, rec = _serial(model, x)
    assert rec == (count, _latency(count, ncu))
