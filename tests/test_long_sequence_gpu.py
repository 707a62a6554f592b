"""Sequences up to the 256-step limit against the float64 oracle: the counterpart of test_large_batch_gpu.py on the frame axis.
The model entry points accept 8 <= t_frames <= 2055 (S = t_frames / 8 <= ATT_MAX_S = 256 GRU steps, csrc/model_shape.h); a
512 / 160 / 400 front-end turns a 20 s utterance into 2001 frames.

The module is ordered by sequence length -- the refusals (no kernel runs), then T = 520 (S = 65), 1031, 2047 / 2048 / 2055
(S = 255 / 256 / 256), then the sequences that move between lengths -- so that S = 65 has run before anything at S = 256.
No `dbg` fault-injection bits and no environment switches.

What each (B, T) lands on (csrc/model_shape.h, wino2_geo.h, train_workspace.h, wgrad_wino_f16x3_kernel.h, gru_quad.hip; 256 CUs).
wp1 / wp2 = map widths behind conv1 / conv2, S = GRU steps; TW = Winograd tile columns of conv2 / conv3 (the W2Div divisors
TW and 2 TW; odd wp1 / wp2 leave a half-filled last tile column); K = B * S tokens; ksplits 1 / 2 / 8 below 256 / below 2048 /
from 2048 tokens; dx_splitk (the layer-input gradient as two K halves) for 48 <= tiles < 160, tiles = ceil(K / 128) * in / 256;
nsplit = K splits of tn_dw_plan; strips = wgrad_wino_strips of conv2 / conv3 (caps 128 / 64); stat = Winograd spatial tasks of
conv2 / conv3 before wino2_stat_blocks caps them at the CU count; loss scale = sir_bwd_loss_scale (the batch alone); clusters
of the recurrences (x 4 workgroups); k2max / k3max = 4-column tasks per image of the pad-skip / ragged lists.

    B   T     wp1 / wp2 / S     TW         K     ksplits  dx_splitk l0 / l1  nsplit  strips    stat tasks     loss scale  clusters  k2max / k3max
    5   520   260 / 130 / 65    130 / 65   325   2        no  / no           4 / 6   128 / 64  326* / 82      2^11        2         33 / 17
    5   1031  515 / 257 / 128   258 / 129  640   2        no  / no           4 / 7   128 / 64  646* / 162     2^11        2         65 / 33
    5   2047  1023 / 511 / 255  512 / 256  1275  2        no  / no           4 / 7   128 / 64  1280* / 320*   2^11        2         128 / 64
    5   2048  1024 / 512 / 256  512 / 256  1280  2        no  / no           4 / 7   128 / 64  1280* / 320*   2^11        2         128 / 64
    2   2048  1024 / 512 / 256  512 / 256  512   2        no  / no           4 / 6   128 / 64  512* / 128     2^9         2         128 / 64
    3   2055  1027 / 513 / 256  514 / 257  768   2        no  / no           4 / 6   128 / 64  772* / 193     2^10        2         129 / 65
    5   2055  1027 / 513 / 256  514 / 257  1280  2        no  / no           4 / 7   128 / 64  1286* / 322*   2^11        2         129 / 65
    8   2048  1024 / 512 / 256  512 / 256  2048  8        yes / no           4 / 7   128 / 64  2048* / 512*   2^11        2         128 / 64
    17  2055  1027 / 513 / 256  514 / 257  4352  8        yes / yes          4 / 7   128 / 64  4370* / 1093*  2^13        4         129 / 65
    (8 at t = 200, the short step of the moving test: 100 / 50 / 25, 50 / 25, K = 200, ksplits 1, no / no, 4 / 7, 128 / 64, 200 / 50, 2^11, 2)
    * capped at the CU count.
    (the training columns -- ksplits to loss scale -- apply to the training cases (5, 520), (2, 2048), (3, 2055), (8, 2048); 17 rows run in
    inference only: their second GRU group holds one clip.)

Both sides of ksplits 2 | 8 are reached by length rather than batch ((2, 2048) and (8, 2048)), dx_splitk of layer 0 off | on;
T = 2055 has an odd last tile column at both Winograd stages and the non-power-of-two divisors 514 / 1028 and 257 / 514, T = 2047 /
2048 the power-of-two ones; S = 255 | 256 is the edge of the attention kernels' LDS arrays (`if (tid < S)` uses all 256 threads at
256 only) and step 256 the only one that sets bit 8 of the 9-bit step field of a recurrence exchange tag.  The loss scale depends on
the batch alone: at B = 2, S = 256 the scaled intermediate gradients sit at 2^-5 .. 2^-7 (float64 oracle: rms 2.6e-2 dy1, 1.8e-2
dy0, 1.1e-2 dx0, 8.3e-3 da2, 7.4e-3 da1), ten times lower than at B = 8, T = 200; the five stage gradients are therefore held to
the parameter gradients' bound here as well.

Data: one 17 x 64 x 2055 array (cases.varied_features, seed 2055); a case at T is its first T columns.  References:
oracle/model_ref.py in float64 (state dict and input cast to double), computed once per T in the module fixture (about 10 s on the
CPU in all: the sharp head shares the trunk of the init-scale one and only the classifier is applied twice).

Inference bounds are the neighbours': 2e-5 on init-scale weights, 2e-3 + identical argmax on cases.sharp_head (test_model_gpu.py;
the oracle's top-2 margin is asserted to exceed twice the tolerance, so that the argmax is decided), 1e-4 * max(1, |b|) on the stage
views (test_stages_vs_oracle), bit-identity of +0.0 against -0.0 tails (test_pad_skip_gpu.py), 2e-4 and the argmax wherever the
oracle's margin is >= 1e-3 for the ragged call with at least half the rows clear (test_large_batch_gpu.py), the feature tolerance
and 1e-4 * max(1, |b|) end to end (test_frontend_cfg_gpu.py::test_end_to_end_at_hop_160).  Training bounds are
train_step_ref._training_case's, unchanged: loss 2e-5, logits 5e-5, all 29 gradients and the five stage gradients 2e-3 * rms,
norms 1e-3, BN running statistics rtol 1e-4, the input gradient input_grad_ref.GRAD_BOUND.  Each case prints its figures before it
asserts.

One bound is restated, for one tensor at one shape.  d(loss) / d(attention.bias) is zero in exact arithmetic (a softmax does not
see a shift of its scores), so its norm bound |norm - ref| <= 1e-3 * ref + 1e-7 is the absolute 1e-7 alone, and what either side
computes is the rounding of sum_t w_t (dw_t - sum_t w_t dw_t): about sum_b <w, dw>_b (1 - sum_t w_t), which grows with 1 / B
(d logits) and with S (the 256-term normalisation).  At (2, 2048) the float32 oracle itself, at the device's forward values, gives
|attention.bias gradient| = 1.388e-7 against the float64 oracle's 4.3e-17 -- farther than the bound -- and the device 1.178e-7.
The absolute term for that tensor at that shape is therefore 4 x 1.388e-7 = 5.55e-7; every other tensor and shape keeps 1e-7
(measured for this tensor: (5, 520) device 1.2e-8 / float32 7.3e-9, (3, 2055) 3.8e-8 / 5.9e-9, (2, 2048) with dropout
4.0e-8 / 5.5e-8, (8, 2048) 3.3e-8 / 2.2e-8).  No other bound was widened."""
import ctypes as C

import numpy as np
import pytest
import torch

import cases
import frontend_cfg_ref
from oracle import model_ref
from sir_amd import _native, featurizer, ops, synth, train_ops
from sir_amd.featurizer import get_featurizer
from sir_amd.models.models import CNNAudioGRU
from train_step_ref import _training_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
TMAX = 2055
NROWS = 17
TS = (24, 520, 1031, 2047, 2048, 2055)                  # 24: the short call of the moving tests
RAGGED_TOL, RAGGED_MARGIN = 2e-4, 1e-3
# data extents of rows 0..12 of the +0.0-tails batch at T = 2055 and the live GRU steps the pad skip must find for them
TAIL_EXTENTS = [1, 2, 3, 9, 10, 1023, 1024, 2033, 2034, 2041, 2042, 2047, 2054]
TAIL_STEPS = [1, 2, 2, 2, 3, 129, 129, 255, 256, 256, 256, 256, 256]
# un-padded lengths at t_frames = 2055: 1-step and 256-step clips in one cluster, a second cluster with one clip
RAGGED_FRAMES = [8, 9, 15, 16, 23, 2055, 2048, 2047, 2040, 1031, 1024, 520, 333, 1999, 2054, 100, 64]
POSITION_ROWS = [0, 15, 16]
MOVE_TS = (2055, 24, 2048, 520, 2055)
ATTN_BIAS_ATOL_2X2048 = 4 * 1.388e-7                    # (module docstring: the one restated bound)


def _f64(sd):
    return {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in sd.items()}


@pytest.fixture(scope="module")
def sd():
    return synth.synth_state_dict(31, seed=0)


@pytest.fixture(scope="module")
def sharp_sd(sd, model_golden):
    return cases.sharp_head(sd, model_golden["sharp_fc_bias"])


def _rows(t):
    return NROWS if t == TMAX else 5


def _head(sd64, ctx):
    return ctx @ sd64["fc.weight"].t() + sd64["fc.bias"]


@pytest.fixture(scope="module")
def data(sd, sharp_sd):
    """The 17 clips and their float64 oracle logits, computed once.  In eval mode a row does not see its batch, so a batch of B
    is the first B rows of the reference of its T.  cases.sharp_head changes the classifier alone: its logits are that
    classifier on the oracle's context vectors."""
    x = cases.varied_features(NROWS, TMAX, seed=2055).float()
    sd64, sharp64 = _f64(sd), _f64(sharp_sd)
    for k in sd64:
        assert k in ("fc.weight", "fc.bias") or torch.equal(sd64[k], sharp64[k]), k
    xz = x.clone()
    for b, e in enumerate(TAIL_EXTENTS):
        xz[b, :, e:] = 0.0
    xn = x.clone()
    for b, f in enumerate(RAGGED_FRAMES):
        xn[b, :, f:] = float("nan")
    ref, ref_sharp, stages = {}, {}, {}
    with torch.no_grad():
        for t in TS:
            st = {}
            ref[t] = model_ref.forward(sd64, x[:_rows(t), :, :t].double(), stages=st)
            ref_sharp[t] = _head(sharp64, st["ctx"])
            if t == TMAX:
                stages = {k: v[:3] for k, v in st.items()}
        ref_tails = ref[TMAX].clone()
        n = len(TAIL_EXTENTS)
        ref_tails[:n] = model_ref.forward(sd64, xz[:n].double())
        ref_ragged = torch.cat([model_ref.forward(sd64, x[b:b + 1, :, :f].double()) for b, f in enumerate(RAGGED_FRAMES)])
    return {"x": x, "xz": xz, "xn": xn, "ref": ref, "ref_sharp": ref_sharp, "stages": stages, "ref_tails": ref_tails,
            "ref_ragged": ref_ragged}


def _eval_model(sd):
    m = CNNAudioGRU(31)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def _train_model(sd, dropout=0.0):
    m = CNNAudioGRU(31)
    m.load_state_dict(sd)
    m = m.to(DEV).train()
    m.gru.dropout = dropout
    return m


def _infer(m, x, ws=None, **kw):
    lg, am = ops.model_infer(m, x, ws if ws is not None else ops.Workspace(), want_argmax=True, **kw)
    torch.cuda.synchronize()
    return lg, am


def _ws_bytes(bsz, t, train=0):
    return _native.lib().sir_model_workspace_bytes(get_featurizer().handle, bsz, t, train)


def _ff_workspace(bsz, t):
    ws = ops.Workspace()
    ws.get(_ws_bytes(bsz, t), torch.device(DEV, torch.cuda.current_device())).fill_(0xFF)
    return ws


def _neg_tail(x):
    """the same features with the all-+0.0 tail of every utterance replaced by -0.0 (forces the full path)"""
    nz = (x.view(torch.int32) != 0).any(dim=1)
    e0 = (nz * (torch.arange(x.shape[2], device=x.device) + 1)).amax(dim=1)
    tail = (torch.arange(x.shape[2], device=x.device)[None, None, :] >= e0[:, None, None]).expand_as(x)
    return torch.where(tail, torch.full_like(x, -0.0), x)


def _scribble(buf):
    """test_robustness_gpu.py's, with the whole step field: float bit patterns whose top 16 bits are plausible forward-granule
    tags {7-bit epoch, 9-bit step + 1} -- steps 1..256 (bit 8 of the field set at 256) under each of the 128 epochs in turn --
    then the prepared weights kept in the workspace are invalidated."""
    v = buf[: buf.numel() & ~3].view(torch.int32)
    i = torch.arange(v.numel(), device=buf.device, dtype=torch.int64)
    tag = (((i >> 8) & 127) << 9) | (i % 256 + 1)
    bits = (tag << 16) | 0x1234
    v.copy_(torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(torch.int32))
    ops.bump_weights_epoch()


def _margin(ref):
    top2 = ref.topk(2, dim=1).values
    return top2[:, 0] - top2[:, 1]


def _maxerr(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return ((a - b).abs() / b.abs().clamp(min=1.0)).max().item()


# ---- refusals: no kernel runs ---------------------------------------------------------------------------------------------
BAD_SHAPES = [(2, 7), (2, 2056), (65536, 8)]


def test_shapes_outside_the_range_are_refused_by_the_c_entry_points(sd):
    """t_frames 7 and 2056 and batch 65536: sir_model_workspace_bytes returns 0 for both `train` values, the launch entry points
    SIR_EINVAL with the real limits in the message and the logits untouched, the offsets calls SIR_EINVAL; 8 and 2055 frames are
    accepted."""
    lib, h = _native.lib(), get_featurizer().handle
    m = _eval_model(sd)
    w, _keep = ops.cached_weights(m)
    rm = (C.c_void_p * 3)(*[getattr(m, f"bn{i}").running_mean.data_ptr() for i in (1, 2, 3)])
    rv = (C.c_void_p * 3)(*[getattr(m, f"bn{i}").running_var.data_ptr() for i in (1, 2, 3)])
    stats0 = [getattr(m, f"bn{i}").running_mean.clone() for i in (1, 2, 3)]
    cfg = train_ops.bn_config(_train_model(sd))
    nws = max(_ws_bytes(2, TMAX, 0), _ws_bytes(2, TMAX, 1))
    assert nws > 0
    ws = torch.zeros(nws, dtype=torch.uint8, device=DEV)
    stream = _native.current_stream_ptr()
    offs = (C.c_size_t * 40)()
    for bsz, t in BAD_SHAPES:
        assert lib.sir_model_workspace_bytes(h, bsz, t, 0) == 0, (bsz, t)
        assert lib.sir_model_workspace_bytes(h, bsz, t, 1) == 0, (bsz, t)
        feats = torch.zeros(bsz, 64, t, device=DEV)      # (whole: a call that was not refused would read valid memory)
        frames = torch.full((bsz,), 8, dtype=torch.int32, device=DEV)
        logits = torch.full((bsz, 31), -7.0, device=DEV)
        calls = {
            "sir_model_infer": lambda: lib.sir_model_infer(h, C.byref(w), feats.data_ptr(), bsz, t, logits.data_ptr(), None,
                                                           ws.data_ptr(), ws.numel(), stream),
            "sir_model_infer_ragged": lambda: lib.sir_model_infer_ragged(h, C.byref(w), feats.data_ptr(), frames.data_ptr(), bsz, t,
                                                                         logits.data_ptr(), None, ws.data_ptr(), ws.numel(), stream),
            "sir_model_train_fwd": lambda: lib.sir_model_train_fwd_cfg(h, C.byref(w), rm, rv, feats.data_ptr(), bsz, t, 0.1, 0.0, 0,
                                                                       C.byref(cfg), logits.data_ptr(), ws.data_ptr(), ws.numel(), stream),
        }
        for who, call in calls.items():
            assert call() == _native.SIR_EINVAL, (who, bsz, t)
            msg = lib.sir_last_error().decode()
            assert who in msg and "2055" in msg and "65535" in msg and f"t_frames={t}" in msg, msg
        assert lib.sir_model_workspace_offsets(h, bsz, t, 0, offs, 16) == _native.SIR_EINVAL
        assert "2055" in lib.sir_last_error().decode()
        assert lib.sir_model_train_workspace_offsets(h, bsz, t, offs, 40) == _native.SIR_EINVAL
        assert "2055" in lib.sir_last_error().decode()
        torch.cuda.synchronize()
        assert (logits == -7.0).all(), (bsz, t)
        del feats, logits
    for i, s0 in enumerate(stats0):
        assert torch.equal(getattr(m, f"bn{i + 1}").running_mean, s0)
    for t in (8, TMAX):                                  # both ends of the range are accepted
        assert lib.sir_model_workspace_bytes(h, 2, t, 0) > 0 and lib.sir_model_workspace_bytes(h, 2, t, 1) > 0
        assert lib.sir_model_workspace_offsets(h, 2, t, 0, offs, 16) > 0
        assert lib.sir_model_train_workspace_offsets(h, 2, t, offs, 40) > 0
    assert lib.sir_model_workspace_bytes(h, 65535, 8, 0) > 0
    ops.check_status()


@pytest.mark.parametrize("bsz,t", BAD_SHAPES)
def test_shapes_outside_the_range_are_refused_through_python(sd, bsz, t):
    x = torch.zeros(bsz, 64, t, device=DEV)
    m = _eval_model(sd)
    with pytest.raises(_native.SirError, match="2055"):
        m.predict(x)
    with pytest.raises(_native.SirError, match="2055"):
        m.predict(x, lengths=torch.full((bsz,), min(t, 8), dtype=torch.int32, device=DEV))
    mt = _train_model(sd)
    with pytest.raises(_native.SirError, match="2055"):
        mt(x)
    ops.check_status()


# ---- inference against the oracle, by length --------------------------------------------------------------------------------
def _dense_case(t, bsz, sd, sharp_sd, data):
    x = data["x"][:bsz, :, :t].contiguous().to(DEV)
    ref, ref_sharp = data["ref"][t][:bsz], data["ref_sharp"][t][:bsz]
    lg, am = _infer(_eval_model(sd), x)
    err = (lg.cpu().double() - ref).abs().max().item()
    lgs, ams = _infer(_eval_model(sharp_sd), x)
    errs = (lgs.cpu().double() - ref_sharp).abs().max().item()
    print(f"T={t} B={bsz} dense: max |logit error| {err:.2e} (init scale; smallest oracle margin {_margin(ref).min().item():.2e}), "
          f"{errs:.2e} (sharp head; smallest oracle margin {_margin(ref_sharp).min().item():.2e})")
    assert _margin(ref).min().item() > 2 * 2e-5 and _margin(ref_sharp).min().item() > 2 * 2e-3      # the argmax is decided
    assert err <= 2e-5
    assert torch.equal(am.cpu(), lg.cpu().argmax(1)) and torch.equal(am.cpu(), ref.argmax(1))
    assert errs < 2e-3
    assert torch.equal(ams.cpu(), ref_sharp.argmax(1))
    ops.check_status()


@pytest.mark.parametrize("t", [520, 1031, 2047, 2048, 2055])
def test_dense_inference_vs_oracle(sd, sharp_sd, data, t):
    _dense_case(t, 5, sd, sharp_sd, data)


def test_dense_inference_vs_oracle_17_rows_at_2055(sd, sharp_sd, data):
    """all 17 rows: a second, nearly empty GRU group (one clip in a cluster of 16) beside a full one, K = 4352 tokens"""
    _dense_case(TMAX, NROWS, sd, sharp_sd, data)


def test_stages_vs_oracle_at_2055(sd, data):
    """test_model_gpu.py::test_stages_vs_oracle at B = 3, T = 2055: widths 1027 / 513 / 256"""
    m = _eval_model(sd)
    dbg = {}
    logits = ops.model_infer(m, data["x"][:3].contiguous().to(DEV), m._ws, debug=dbg)
    torch.cuda.synchronize()
    st = data["stages"]
    errs = {
        "conv1": _maxerr(dbg["conv1"], st["conv1"].permute(0, 2, 3, 1)),
        "conv2": _maxerr(dbg["conv2"], st["conv2"].permute(0, 2, 3, 1)),
        "gru_in": _maxerr(dbg["gru_in"], st["gru_in"]),
        "gru_l0": _maxerr(dbg["gru_l0"], st["gru_l0"]),
        "gru_l1": _maxerr(dbg["gru_l1"], st["gru_l1"]),
        "ctx": _maxerr(dbg["ctx"], st["ctx"]),
        "logits": _maxerr(logits, data["ref"][TMAX][:3]),
    }
    print("T=2055 B=3 stage max rel-abs errors:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert dbg["conv1"].shape == (3, 32, 1027, 32) and dbg["conv2"].shape == (3, 16, 513, 64) and dbg["gru_l1"].shape == (3, 256, 512)
    for k, v in errs.items():
        assert v <= 1e-4, (k, v, errs)
    ops.check_status()


def test_zero_tails_at_2055_vs_oracle(sd, data):
    """+0.0 tails from 1 to 2054 columns of data (1 to 256 live GRU steps) in one batch of 17: the pad skip finds the issue's step
    counts, the result is bit-identical to the -0.0-tail (full) computation, both on 0xFF-filled workspaces, and within 2e-5 of
    the oracle."""
    m = _eval_model(sd)
    x = data["xz"].to(DEV)
    xf = _neg_tail(x)
    assert not torch.equal(x.view(torch.int32), xf.view(torch.int32))
    ws = _ff_workspace(NROWS, TMAX)
    lg, am = _infer(m, x, ws)
    tabs = ops.pad_skip_tables(ws.buf, NROWS, TMAX)
    lgf, amf = _infer(m, xf, _ff_workspace(NROWS, TMAX))
    assert tabs["e0"].tolist() == TAIL_EXTENTS + [TMAX] * (NROWS - len(TAIL_EXTENTS))
    d3 = tabs["d3"].tolist()
    assert d3[:len(TAIL_STEPS)] == TAIL_STEPS and d3[len(TAIL_STEPS):NROWS] == [256] * (NROWS - len(TAIL_STEPS)) and d3[NROWS] == 256
    assert torch.equal(lg.view(torch.int32), lgf.view(torch.int32)) and torch.equal(am, amf)
    ref = data["ref_tails"]
    err = (lg.cpu().double() - ref).abs().max().item()
    print(f"T=2055 B=17 +0.0 tails: bit-identical to -0.0 tails, max |logit error| {err:.2e} (smallest oracle margin {_margin(ref).min().item():.2e})")
    assert ref.isfinite().all() and _margin(ref).min().item() > 2 * 2e-5
    assert err <= 2e-5
    assert torch.equal(am.cpu(), ref.argmax(1))
    ops.check_status()


def test_ragged_at_2055_vs_oracle(sd, data):
    """1-step and 256-step clips in one cluster: NaN behind each clip's length, a 0xFF-filled workspace, every reference row the
    clip alone at its own length."""
    m = _eval_model(sd)
    lg, am = _infer(m, data["xn"].to(DEV), _ff_workspace(NROWS, TMAX),
                    lengths=torch.tensor(RAGGED_FRAMES, dtype=torch.int32, device=DEV))
    lg, am, ref = lg.cpu(), am.cpu(), data["ref_ragged"]
    assert not lg.isnan().any()
    err = (lg.double() - ref).abs().max().item()
    clear = _margin(ref) >= RAGGED_MARGIN
    print(f"T=2055 B=17 ragged: max |logit error| {err:.2e}, {int((~clear).sum())} clips below the argmax margin "
          f"(smallest oracle margin {_margin(ref).min().item():.2e})")
    assert err <= RAGGED_TOL
    assert torch.equal(am[clear], ref.argmax(1)[clear])
    assert int(clear.sum()) >= NROWS // 2
    ops.check_status()


def test_position_independence_at_2055(sd, data):
    """rows 0, 15 and 16 of the 17-row batch (first of the full cluster, its last, the lone clip of the second one) run alone as a
    3-row batch: bit-identical, dense and with the +0.0 tails"""
    m = _eval_model(sd)
    for key in ("x", "xz"):
        x = data[key].to(DEV)
        lg, am = _infer(m, x)
        lgr, amr = _infer(m, x[POSITION_ROWS].contiguous())
        assert torch.equal(lgr.view(torch.int32), lg[POSITION_ROWS].view(torch.int32)) and torch.equal(amr, am[POSITION_ROWS]), key
    ops.check_status()


def test_end_to_end_20_s_at_hop_160(sd):
    """test_frontend_cfg_gpu.py::test_end_to_end_at_hop_160 on two 20 s clips: 2001 frames at t_pad 2004 (S = 250)."""
    fz = featurizer.get_featurizer(16000, 64, 512, 160, 400)
    wave = synth.synth_clips(2, 320000, seed=2001)
    feats = fz(wave.to(DEV), t_pad=2004)
    logits, pred = _eval_model(sd).predict(feats)
    torch.cuda.synchronize()
    assert frontend_cfg_ref.num_frames(320000, 512, 160) == 2001
    r_feats, _ = frontend_cfg_ref.batch_f32(list(wave), 512, 160, 400, 2004)
    f, r = feats.cpu().double().numpy(), r_feats.double().numpy()
    ferr = (np.abs(f - r) / np.maximum(1.0, np.abs(r))).max()
    with torch.no_grad():
        r_logits = model_ref.forward(_f64(sd), feats.cpu().double())
    err = _maxerr(logits, r_logits)
    print(f"20 s at hop 160 (2001 frames): features max rel-abs error {ferr:.2e}, logits max rel-abs error {err:.2e}")
    assert (f[:, :, 2001:] == 0).all() and np.abs(f[:, :, 2000]).max() > 0
    assert ferr <= 1e-4
    assert err <= 1e-4
    assert torch.equal(pred.cpu(), r_logits.argmax(1))
    ops.check_status()


# ---- training against the oracle, by length ---------------------------------------------------------------------------------
def test_training_step_vs_oracle_5x520(sd):
    print("T=520:")
    _training_case(sd, 5, 520)


def test_training_step_vs_oracle_2x2048(sd):
    """K = 512 at the smallest loss scale a 256-step clip can meet in a batch of two (2^9).  The absolute term of attention.bias's
    norm bound is restated here (module docstring): 4 x the float32 oracle's own 1.388e-7 instead of 1e-7."""
    print("T=2048:")
    _training_case(sd, 2, 2048, norm_atol={"attention.bias": ATTN_BIAS_ATOL_2X2048})


def test_training_step_vs_oracle_3x2055_with_input_gradient(sd):
    """odd widths 1027 / 513 with ``dfeats`` requested (sir_model_train_bwd_x)"""
    print("T=2055:")
    _training_case(sd, 3, 2055, want_dx=True)


def test_training_step_vs_oracle_2x2048_with_dropout(sd):
    """the keep mask rebuilt on the host, checked bit for bit against y0d, fed to the oracle.  The mask is the one of dropout
    step 4 whatever ran before this test in the process (the counter is put back afterwards), so that the case is one fixed
    input like the others."""
    print("T=2048:")
    step = train_ops.dropout_step()
    train_ops.set_dropout_step(4)
    try:
        _training_case(sd, 2, 2048, dropout=0.5)
    finally:
        train_ops.set_dropout_step(step + 1)


def test_training_step_vs_oracle_8x2048(sd):
    """K = 2048: the ksplits 2 | 8 boundary reached by length rather than batch.  (The float32 oracle's own distance is not
    computed here, to save its 2 s: at the device's forward values it is 1.5e-4 * rms on its worst gradient, conv1.weight.)"""
    print("T=2048:")
    _training_case(sd, 8, 2048, compare_f32=False)


def _c_backward(m, x, dlogits, parts):
    """test_large_batch_gpu.py's: direct C calls of the backward (one per entry of ``parts``) on the workspace ``m``'s last forward
    left, all 29 gradients into a buffer of its own."""
    lib, h = _native.lib(), get_featurizer().handle
    buf = train_ops.GradBuffer(m)
    w, _keep = ops.cached_weights(m)
    seed, p = m._sir_last_dropout
    ws = m._sir_train["ws"].buf
    for part in parts:
        rc = lib.sir_model_train_bwd_cfg(h, C.byref(w), x.data_ptr(), dlogits.data_ptr(), x.shape[0], x.shape[-1], p, seed,
                                         C.byref(train_ops.bn_config(m)), C.byref(buf.struct), ws.data_ptr(), ws.numel(), part,
                                         _native.current_stream_ptr())
        _native.check(rc, "sir_model_train_bwd_cfg")
    torch.cuda.synchronize()
    return buf.flat


def test_backward_in_two_parts_is_bit_identical_at_3x2055(sd):
    """SIR_BWD_HEAD_GRU then SIR_BWD_CNN against the single call (and against autograd's): all 29 gradients bit-identical."""
    lib, h = _native.lib(), get_featurizer().handle
    bsz = 3
    x = cases.varied_features(bsz, TMAX, seed=4000).to(DEV)
    y = synth.synth_labels(bsz, 31, seed=4001).to(DEV)
    m = _train_model(sd)
    m.zero_grad(set_to_none=True)
    train_ops.fused_cross_entropy(m(x), y).backward()
    torch.cuda.synchronize()
    auto = torch.cat([p.grad.flatten() for p in m.parameters()]).clone()
    assert auto.abs().max() > 0
    logits = m(x)                                        # (the running statistics move; the batch statistics and gradients do not)
    dlogits, loss = torch.empty_like(logits), torch.empty((), device=DEV)
    _native.check(lib.sir_ce_loss(h, logits.data_ptr(), y.data_ptr(), bsz, 31, loss.data_ptr(), dlogits.data_ptr(), 1.0,
                                  _native.current_stream_ptr()), "sir_ce_loss")
    whole = _c_backward(m, x, dlogits, [_native.BWD_ALL])
    halves = _c_backward(m, x, dlogits, [_native.BWD_HEAD_GRU, _native.BWD_CNN])
    assert torch.equal(whole, auto)
    assert torch.equal(halves, whole)
    ops.check_status()


# ---- moving between lengths on one workspace: high-step tags stay behind in the exchange buffers ----------------------------
def _move_frames(t):
    return [8, t, max(8, t - 1), max(8, t // 2), min(t, 9)]


def test_inference_moving_between_lengths(sd, data):
    """T = 2055, 24, 2048, 520, 2055 on one ops.Workspace and one model, the workspace scribbled before every call: each result is
    bit-identical to the same call on a fresh workspace (and within 2e-5 of the oracle).  A short launch after a long one, and
    the reverse, finds granules of steps it never reaches under an older epoch.  Then the same sequence through the ragged
    entry point, 1-step and full-length clips together."""
    fresh, fresh_ragged, xs, xr, lens = {}, {}, {}, {}, {}
    for t in sorted(set(MOVE_TS)):
        xs[t] = data["x"][:5, :, :t].contiguous().to(DEV)
        fr = _move_frames(t)
        xr[t] = xs[t].clone()
        for b, f in enumerate(fr):
            xr[t][b, :, f:] = float("nan")
        lens[t] = torch.tensor(fr, dtype=torch.int32, device=DEV)
        fresh[t] = _infer(_eval_model(sd), xs[t])
        fresh_ragged[t] = _infer(_eval_model(sd), xr[t], lengths=lens[t])
        assert not fresh_ragged[t][0].isnan().any()
        assert (fresh[t][0].cpu().double() - data["ref"][t][:5]).abs().max().item() <= 2e-5, t
    m = _eval_model(sd)
    ws = ops.Workspace()
    ws.get(_ws_bytes(5, TMAX), xs[TMAX].device)
    for ragged in (False, True):
        for step, t in enumerate(MOVE_TS):
            _scribble(ws.buf)
            if ragged:
                lg, am = _infer(m, xr[t], ws, lengths=lens[t])
                want = fresh_ragged[t]
            else:
                lg, am = _infer(m, xs[t], ws)
                want = fresh[t]
            assert torch.equal(lg.view(torch.int32), want[0].view(torch.int32)) and torch.equal(am, want[1]), (ragged, step, t)
    ops.check_status()


def test_training_moving_between_lengths(sd):
    """One step at (2, 2048), one at (8, 200), then (2, 2048) again on the same model object, the workspace scribbled in between:
    loss and all 29 gradients of the third step are bit-identical to the first's (the method of
    test_large_batch_gpu.py::test_training_moving_between_small_and_large_batches)."""
    m = _train_model(sd)
    batches = {(b, t): (cases.varied_features(b, t, seed=5000 + t).to(DEV), synth.synth_labels(b, 31, seed=t).to(DEV))
               for b, t in ((2, 2048), (8, 200))}
    first = {}
    for step, key in enumerate(((2, 2048), (8, 200), (2, 2048), (8, 200))):
        x, y = batches[key]
        for p in m.parameters():
            p.grad = None
        m.load_state_dict(sd)                            # the same weights and BN buffers every time
        loss = train_ops.fused_cross_entropy(m(x), y)
        loss.backward()
        torch.cuda.synchronize()
        g = torch.cat([p.grad.flatten() for p in m.parameters()]).clone()
        assert g.isfinite().all() and g.abs().max() > 0
        if key not in first:
            first[key] = (loss.detach().clone(), g)
        assert torch.equal(loss.detach(), first[key][0]), (step, key)
        assert torch.equal(g, first[key][1]), (step, key)
        _scribble(m._sir_train["ws"].buf)
    ops.check_status()
