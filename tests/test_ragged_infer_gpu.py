"""Un-padded ("ragged") batch inference: sir_model_infer_ragged through ops.model_infer(..., lengths=...).

Row b of a ragged call must be what the model gives clip b ALONE at its own length -- CNNAudioGRU.forward(x[b:b+1, :, :frames[b]])
in eval mode, the way the reference's scripts/test_tts_samples.py feeds every file -- and not the padded function, which differs from
it by 2.6e-3 to 0.2 on these inputs.  Every feature column behind a clip's length is NaN and the workspace is filled with NaN bit
patterns before each call: nothing the result depends on may be read from either.

Tolerances: logits within 2e-4 of the CPU oracle (the bound of tests/test_model_gpu.py: sums of up to 1024 fp32 products in another
order), argmax identical wherever the oracle's top-2 margin is >= 1e-3 (at most one clip may fall below; the oracle's margins here
start 3.7e-4, 1.2e-3, 1.5e-3, ...).  Measured on MI355X: see test_matches_oracle_clip_by_clip's docstring."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cases
from oracle import model_ref
from sir_amd import _native, ops, synth
from sir_amd.featurizer import get_featurizer
from sir_amd.models.models import CNNAudioGRU

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = [8, 9, 15, 16, 17, 23, 31, 32, 33, 47, 63, 64, 94, 95, 120, 199, 200, 8, 200, 94, 13, 77, 150, 40, 24, 25, 100, 101, 55, 8,
          200, 12, 187]
TOL = 2e-4
MARGIN = 1e-3


def _model(sd):
    m = CNNAudioGRU(31)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def _nan_tails(x, frames):
    """a copy of x [B, 64, T] with every column >= frames[b] overwritten with NaN"""
    x = x.clone()
    for b, f in enumerate(frames):
        x[b, :, f:] = float("nan")
    return x


def _ragged(m, x, frames, as_list=False):
    """one ragged call on a NaN-filled workspace -> (logits, argmax) on the CPU"""
    x = x.to(DEV)
    ws = ops.Workspace()
    need = _native.lib().sir_model_workspace_bytes(get_featurizer().handle, x.shape[0], x.shape[-1], 0)
    ws.get(need, x.device).fill_(0xFF)
    lengths = list(frames) if as_list else torch.tensor(frames, dtype=torch.int32, device=DEV)
    lg, am = ops.model_infer(m, x, ws, want_argmax=True, lengths=lengths)
    torch.cuda.synchronize()
    return lg.cpu(), am.cpu()


def _check_rows(lg, am, ref, rows=None):
    """rows of (lg, am) against the oracle rows `ref`: logits within TOL, argmax identical where the oracle's margin >= MARGIN"""
    rows = range(ref.shape[0]) if rows is None else rows
    err, skipped = 0.0, 0
    for i, b in enumerate(rows):
        err = max(err, (lg[i] - ref[b]).abs().max().item())
        top2 = ref[b].topk(2).values
        if (top2[0] - top2[1]).item() >= MARGIN:
            assert int(am[i]) == int(ref[b].argmax()), (b, lg[i], ref[b])
        else:
            skipped += 1
    print(f"ragged vs oracle: max |logit error| {err:.3e} over {len(list(rows))} clips, {skipped} below the argmax margin")
    assert err <= TOL, err
    assert skipped <= 1, skipped
    return err


@pytest.fixture(scope="module")
def sd():
    return synth.synth_state_dict(31, seed=0)


@pytest.fixture(scope="module")
def data(sd):
    """the fixed batch: clean features, the NaN-tailed copy, and the oracle's logits clip by clip (computed once)"""
    x = cases.varied_features(33, 200, seed=11).float()
    with torch.no_grad():
        ref = torch.cat([model_ref.forward(sd, x[b:b + 1, :, :f]) for b, f in enumerate(FRAMES)])
    return {"x": x, "xn": _nan_tails(x, FRAMES), "ref": ref}


def test_matches_oracle_clip_by_clip(sd, data):
    """33 clips, lengths 8 ... 200 (S_b = 1 ... 25, every odd-width drop of the three poolings, two full GRU clusters + 1).
    Measured on MI355X: max |logit error| 2.1e-7 against the bound of 2e-4 (1.9e-7 on the conv fallback kernels); one clip (oracle
    margin 3.7e-4) is below the argmax margin, every other argmax is identical."""
    m = _model(sd)
    lg, am = _ragged(m, data["xn"], FRAMES)
    assert not lg.isnan().any()
    _check_rows(lg, am, data["ref"])
    # the padded function is something else: a call that quietly ran it would be off by orders of magnitude more than TOL
    with torch.no_grad():
        padded = model_ref.forward(sd, torch.nn.functional.pad(data["x"][12:13, :, :94], (0, 106)))
    assert (padded - data["ref"][12:13]).abs().max().item() > 10 * TOL
    ops.check_status()


def test_host_list_of_lengths(sd, data):
    m = _model(sd)
    lg, am = _ragged(m, data["xn"], FRAMES, as_list=True)
    lgt, amt = _ragged(m, data["xn"], FRAMES)
    assert torch.equal(lg, lgt) and torch.equal(am, amt)


def test_row_matches_reference_golden(sd, model_golden):
    """The reference's own output for its un-padded 94-frame clip, reproduced as row 3 of a 5-row ragged batch at t_frames = 200.
    e0 = the error of the existing single-clip call against the same golden values; the ragged row may be off by max(2e-5, 2 e0)
    (another tiling of the same fp32 sums).  Measured on MI355X: e0 = 6.0e-8, ragged row 6.0e-8: the two paths are bit-identical (the test
    prints all three)."""
    inp = cases.model_inputs()
    m = _model(sd)
    x1 = inp["x_eval1_t94"]                                            # [1, 1, 64, 94]
    lg1, _ = m.predict(x1.to(DEV))
    torch.cuda.synchronize()
    gold = torch.from_numpy(np.asarray(model_golden["eval1_logits"]))
    e0 = (lg1.cpu() - gold).abs().max().item()
    frames = [200, 37, 8, 94, 150]
    x = inp["x_eval8"][:5].clone()
    x[3, :, :94] = x1[0, 0]
    lg, am = _ragged(m, _nan_tails(x, frames), frames)
    e = (lg[3:4] - gold).abs().max().item()
    same = torch.equal(lg[3:4], lg1.cpu())
    print(f"golden eval1: single-clip error e0 {e0:.3e}, ragged row error {e:.3e}, bit-identical to the single-clip call: {same}")
    assert e <= max(2e-5, 2 * e0), (e, e0)
    assert int(am[3]) == int(model_golden["eval1_argmax"][0])


def test_independent_of_the_batch_around_a_clip(sd, data):
    m = _model(sd)
    ref = data["ref"]
    lg, am = _ragged(m, data["xn"], FRAMES)
    lg2, am2 = _ragged(m, data["xn"], FRAMES)
    assert torch.equal(lg.view(torch.int32), lg2.view(torch.int32)) and torch.equal(am, am2)      # the identical batch: bit-identical
    perm = torch.randperm(33, generator=torch.Generator().manual_seed(3))
    lgp, amp = _ragged(m, data["xn"][perm].contiguous(), [FRAMES[i] for i in perm.tolist()])
    assert (lgp - lg[perm]).abs().max().item() <= TOL
    assert torch.equal(amp, am[perm])
    print("permuted batch bit-identical:", torch.equal(lgp, lg[perm]))
    # the first 5 clips alone in a 37-frame batch, lengths clipped to 37 (all five are shorter: the same clips)
    f5 = [min(f, 37) for f in FRAMES[:5]]
    assert f5 == FRAMES[:5]
    lg5, am5 = _ragged(m, _nan_tails(data["x"][:5, :, :37].contiguous(), f5), f5)
    assert (lg5 - lg[:5]).abs().max().item() <= TOL
    assert torch.equal(am5, am[:5])
    _check_rows(lg5, am5, ref, rows=range(5))


@pytest.mark.parametrize("bsz,t", [(1, 200), (5, 37)])
def test_full_width_equals_padded_call(sd, bsz, t):
    m = _model(sd)
    x = cases.varied_features(bsz, t, seed=13).float().to(DEV)
    lgr, amr = _ragged(m, x, [t] * bsz)
    lgp, amp = ops.model_infer(m, x, ops.Workspace(), want_argmax=True)
    torch.cuda.synchronize()
    assert (lgr - lgp.cpu()).abs().max().item() <= TOL
    assert torch.equal(amr, amp.cpu())


def test_ragged_and_padded_calls_share_prepared_weights(sd, data):
    """calls that differ only in `frames`, and a padded call in between, on ONE workspace: results as on fresh workspaces"""
    m = _model(sd)
    x = data["xn"][:5].to(DEV)
    xp = data["x"][:5].to(DEV)
    fa, fb = FRAMES[:5], [8, 8, 8, 16, 16]
    ws = ops.Workspace()
    a1 = ops.model_infer(m, x, ws, lengths=fa).cpu()
    p1 = ops.model_infer(m, xp, ws).cpu()
    b1 = ops.model_infer(m, x, ws, lengths=fb).cpu()
    a2 = ops.model_infer(m, x, ws, lengths=fa).cpu()
    assert torch.equal(a1, a2)
    assert torch.equal(a1, _ragged(m, x, fa)[0])
    assert torch.equal(b1, _ragged(m, x, fb)[0])
    assert torch.equal(p1, ops.model_infer(m, xp, ops.Workspace()).cpu())


def test_bad_lengths(sd, data):
    m = _model(sd)
    ref = data["ref"]
    frames = list(FRAMES[:8])
    frames[2], frames[5] = 7, 201
    good = [b for b in range(8) if b not in (2, 5)]
    lg, am = _ragged(m, _nan_tails(data["x"][:8], [FRAMES[b] for b in range(8)]), frames)
    assert lg[2].isnan().all() and lg[5].isnan().all()
    assert not lg[good].isnan().any()
    with pytest.raises(_native.SirError):
        ops.check_status()
    ops.check_status()                                                 # the word is cleared by the check that reported it
    _check_rows(lg[good], am[good], ref, rows=good)
    # a host list is validated before anything is launched
    with pytest.raises(_native.SirError):
        ops.model_infer(m, data["x"][:8].to(DEV), ops.Workspace(), lengths=frames)
    with pytest.raises(_native.SirError):
        ops.model_infer(m, data["x"][:8].to(DEV), ops.Workspace(), lengths=FRAMES[:7])
    ops.check_status()


def test_model_surface(sd, data):
    from sir_amd.pipeline import BatchPipeline
    m = _model(sd)
    x = data["xn"][:5].to(DEV)
    f = torch.tensor(FRAMES[:5], dtype=torch.int32, device=DEV)
    lg, am = _ragged(m, x, FRAMES[:5])
    assert torch.equal(m(x, lengths=f).cpu(), lg)
    assert torch.equal(m(x.unsqueeze(1), FRAMES[:5]).cpu(), lg)       # 4-D input, host list
    plg, pam = m.predict(x, lengths=f)
    assert torch.equal(plg.cpu(), lg) and torch.equal(pam.cpu(), am)
    pipe = BatchPipeline(m, n_streams=2)
    outs = [pipe.infer(i, x, lengths=f) for i in range(3)]
    pipe.synchronize()
    for o in outs:
        assert torch.equal(o[0].cpu(), lg) and torch.equal(o[1].cpu(), am)
    m.train()
    with pytest.raises(_native.SirError):
        m(x, lengths=f)
    m.eval()


_CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}, {golden!r}]
import torch
import test_ragged_infer_gpu as t
from sir_amd import synth
import cases
from oracle import model_ref
sd = synth.synth_state_dict(31, seed=0)
frames = t.FRAMES[:17]
x = cases.varied_features(33, 200, seed=11).float()[:17]
with torch.no_grad():
    ref = torch.cat([model_ref.forward(sd, x[b:b + 1, :, :f]) for b, f in enumerate(frames)])
lg, am = t._ragged(t._model(sd), t._nan_tails(x, frames), frames)
t._check_rows(lg, am, ref)
t.ops.check_status()
print("RAGGED-FALLBACK-OK")
"""


def test_fallback_conv_kernels(tmp_path):
    """the first 17 clips on the first-generation / direct conv kernels (SIR_CONV_FALLBACK is read once per process: one fresh
    child per value, each under its own time limit; the second is not started if the first failed)"""
    script = tmp_path / "ragged_fallback.py"
    script.write_text(_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), golden=os.path.join(ROOT, "tests", "golden")))
    for fallback in ("1", "2"):
        env = dict(os.environ, SIR_CONV_FALLBACK=fallback)
        r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, str(script)], capture_output=True, text=True, env=env, cwd=ROOT)
        print(r.stdout[-400:])
        assert r.returncode == 0 and "RAGGED-FALLBACK-OK" in r.stdout, (fallback, r.returncode, r.stdout[-2000:], r.stderr[-3000:])
