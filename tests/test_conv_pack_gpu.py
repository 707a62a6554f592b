"""Leftover packing of the inference conv2 / conv3 task lists (csrc/model_infer.hip, Wino2Geo::ctab in csrc/wino2_geo.h): a last
task with idle tile slots hosts columns of the template utterance or of the next utterance, and the halves of a 128-channel
layer's remaining tasks are dealt one by one.  The logits must be bit-identical to the full-width path, which the same features
with every +0.0 tail replaced by -0.0 force; the lists must hold every demanded column exactly once, in as many tasks as the
packing rule (recomputed here, serially) gives."""
import pytest
import torch

from sir_amd import ops, synth
from sir_amd.models.models import CNNAudioGRU

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = 200
WP2, S = T // 4, T // 8


@pytest.fixture(scope="module")
def model():
    m = CNNAudioGRU(31)
    m.load_state_dict(synth.synth_state_dict(31, seed=0))
    return m.to(DEV).eval()


def _frames_for_d3(v):
    """real frames E0 of an utterance whose GRU steps s < v see data: v = min(S, (E0 + 14) // 8) (head of csrc/infer_tables.h).
    An empty utterance (E0 = 0) has v = 1 as well: conv3 column 0 sees no data then, but it is listed all the same."""
    return 1 if v == 1 else T if v == S else 8 * v - 11


def _feats(frames, seed=3):
    """[B, 64, T] features: non-zero noise in the first frames[b] columns, +0.0 behind them"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(len(frames), 64, T, generator=g) * 2.0 - 4.0
    x = torch.where(x == 0, torch.ones_like(x), x)
    real = torch.arange(T)[None, None, :] < torch.tensor(frames)[:, None, None]
    return torch.where(real, x, torch.zeros_like(x)).to(DEV).contiguous()


def _neg_tail(x, frames):
    cols = torch.arange(T, device=x.device)
    tail = (cols[None, None, :] >= torch.tensor(frames, device=x.device)[:, None, None]).expand_as(x)
    return torch.where(tail, torch.full_like(x, -0.0), x)


def _cap(r):
    return {1: 2, 2: 1}.get(r % 4, 0)


def _pack(needs, tmpl):
    """the packing rule, serially: per image (given away g, guest count, guest's first column as (image, column)), and the task count"""
    q, g, n, plan = 0, 0, 0, []
    for u, c in enumerate(needs):
        r = c - g
        n += (r + 3) // 4
        cap, guest, nxt = _cap(r), None, 0
        if cap and q < tmpl:
            guest = (len(needs), q, min(cap, tmpl - q))
            q += guest[2]
        elif cap and u + 1 < len(needs) and needs[u + 1] > 0:
            nxt = min(cap, needs[u + 1])
            guest = (u + 1, 0, nxt)
        plan.append((g, guest))
        g = nxt
    n += (tmpl - q + 3) // 4
    return n, q, plan


def _check_list(tab, tw, needs, tmpl):
    """tab [n, 2]: the words of every task.  Every demanded column once, segments inside their image and disjoint in the patch"""
    n_rule, q, plan = _pack(needs, tmpl)
    assert tab.shape[0] == n_rule
    seen = {}
    for aw, bw in tab.tolist():
        ga, na = aw >> 2, 1 + (aw & 3)
        segs = [(ga, na)]
        if bw >= 0:
            gb, sb, nb = bw >> 2, 2 + ((bw >> 1) & 1), 1 + (bw & 1)
            assert 2 * na + 2 <= 2 * sb and sb + nb <= 4
            assert gb // tw != ga // tw
            segs.append((gb, nb))
        else:
            assert bw == -1
        for g0, cnt in segs:
            assert (g0 + cnt - 1) // tw == g0 // tw
            for k in range(cnt):
                assert g0 + k not in seen
                seen[g0 + k] = True
    want = {u * tw + c for u, need in enumerate(list(needs) + [tmpl]) for c in range(need)}
    assert set(seen) == want
    return plan


def _run_case(model, frames):
    d3s = [min(S, (e + 14) // 8) for e in frames]
    x = _feats(frames)
    ws = ops.Workspace()
    lg, am = ops.model_infer(model, x, ws, want_argmax=True)
    torch.cuda.synchronize()
    tabs = ops.pad_skip_tables(ws.buf, len(frames), T)
    lgf, amf = ops.model_infer(model, _neg_tail(x, frames), ops.Workspace(), want_argmax=True)
    torch.cuda.synchronize()
    assert tabs["e0"].tolist() == list(frames)
    assert tabs["d3"].tolist() == d3s + [S]
    plan3 = _check_list(tabs["tab3"], (WP2 + 1) // 2, d3s, S)
    plan2 = _check_list(tabs["tab2"], (T // 2 + 1) // 2, [min(WP2, 2 * v + 1) for v in d3s], WP2)
    assert torch.equal(lg, lgf)
    assert torch.equal(am, amf)
    assert not bool(lg.isnan().any())
    return plan2, plan3


def _case(model, d3s):
    return _run_case(model, [_frames_for_d3(v) for v in d3s])


# d3 = 1 three times in a row, 4 (no leftover), 5 (leftover 1: hosts 2), 13 (the benchmark's), 25 (full width, no skip).  Seven
# values do not fit one batch of five: one batch of seven holds them all, and two overlapping batches of five hold them again.
@pytest.mark.parametrize("d3s", [[1, 1, 1, 4, 5, 13, 25], [1, 1, 1, 4, 5], [1, 4, 5, 13, 25]])
def test_every_leftover_kind(model, d3s):
    _case(model, d3s)


def test_chain_after_template_is_used_up(model):
    # 13 hosts of capacity 2 (d3 = 13) take the template's 25 conv3 columns, the last of them one only; the three d3 = 1 images
    # behind them chain: the first hosts the second's only column, so the second lists nothing and hands nothing on, and the
    # third lists its own column with nobody behind it to host
    _, plan3 = _case(model, [13] * 13 + [1, 1, 1])
    assert plan3[12] == (0, (16, 24, 1))
    assert plan3[13] == (0, (14, 0, 1)) and plan3[14] == (1, None) and plan3[15] == (0, None)


def test_chain_through_longer_images(model):
    # no template column is left after the first thirteen; 5 hosts 2 of the next 5, whose other 3 cannot host; 6 - 0 = 6 hosts 1
    # of the 9, whose other 8 leave nothing over; the 2 hosts 1 of the last
    _, plan3 = _case(model, [13] * 13 + [5, 5, 6, 9, 2, 3])
    assert [p[0] for p in plan3[13:]] == [0, 2, 0, 1, 0, 1]


def test_all_empty(model):
    _run_case(model, [0] * 5)


def test_b1_template_is_the_only_guest(model):
    _, plan3 = _case(model, [13])
    assert plan3[0] == (0, (1, 0, 2))


def test_b17_mixed(model):
    _case(model, [13, 1, 1, 1, 4, 5, 13, 25, 1, 2, 6, 9, 10, 13, 3, 7, 22])
