"""The training step from one token to beyond 6400 against the float64 oracle: the token axis K = batch * (t_frames / 8), which
test_large_batch_gpu.py (batch, at t = 24) and test_long_sequence_gpu.py (length, at batch <= 8) each left out.  The model entry
points accept 8 <= t_frames <= 2055 and batch <= 65535, inference and training alike (csrc/model_shape.h).

The module is ordered short end first -- training at 1 to 33 tokens, the backward against itself, inference at 8 to 31 frames --
and the two steps above 6400 tokens last, so that a failure at the short end is seen before the long oracles run.  No `dbg`
fault-injection bits and no environment switches.

What each (B, T) lands on (csrc/model_shape.h, train_workspace.h, wgrad_wino_f16x3_kernel.h, wino2_geo.h; 256 CUs).  S = T / 8 GRU
steps, K = B * S tokens; wp1 / wp2 / wp3 = map widths behind conv1 / conv2 / conv3 (Winograd tile columns of conv2 / conv3:
ceil(wp1 / 2), ceil(wp2 / 2); an odd width leaves a half-filled last tile column); ksplits 1 / 2 / 8 below 256 / below 2048 / from
2048 tokens and kchunk = ceil(K / ksplits) rounded up to the 32-token granule (make_tdims); dx_splitk (the layer-input gradient as
two K halves) for 48 <= tiles < 160, tiles = ceil(K / 128) * in / 256 (below 48 tiles: 64-row tiles, from 160: one pass on 128-row
tiles); nsplit = K splits of tn_dw_plan (each a whole number of 32-token stages: 64 / 32 tokens at the least, caps 4 / 7); strips =
wgrad_wino_strips of conv2 / conv3 over ceil(B * 16 * ceil(wp1 / 2) / 16) / ceil(B * 8 * ceil(wp2 / 2) / 16) stages of 16 tiles (caps
128 / 64, multiples of 8 from 8); loss scale = sir_bwd_loss_scale (the batch alone); clusters of the recurrences = 2 directions x
ceil(B / 16) groups of 16 clips (x 4 workgroups).

    B    T     S    K      wp1 / wp2 / wp3   ksplits  kchunk  dx_splitk l0 / l1  nsplit l0 / l1  strips    loss scale  clusters
    1    8     1    1      4 / 2 / 1         1        32      no  / no           1 / 1           2 / 1     2^8         2
    1    9     1    1      4 / 2 / 1         1        32      no  / no           1 / 1           2 / 1     2^8         2
    2    10    1    2      5 / 2 / 1         1        32      no  / no           1 / 1           6 / 1     2^9         2
    1    12    1    1      6 / 3 / 1         1        32      no  / no           1 / 1           3 / 1     2^8         2
    3    15    1    3      7 / 3 / 1         1        32      no  / no           1 / 1           8 / 3     2^10        2
    1    16    2    2      8 / 4 / 2         1        32      no  / no           1 / 1           4 / 1     2^8         2
    8    16    2    16     8 / 4 / 2         1        32      no  / no           1 / 1           32 / 8    2^11        2
    2    23    2    4      11 / 5 / 2        1        32      no  / no           1 / 1           8 / 3     2^9         2
    1    31    3    3      15 / 7 / 3        1        32      no  / no           1 / 1           8 / 2     2^8         2
    17   8     1    17     4 / 2 / 1         1        32      no  / no           1 / 1           32 / 8    2^13        4
    33   15    1    33     7 / 3 / 1         1        64      no  / no           2 / 2           128 / 32  2^14        6
    (8   200   25   200    100 / 50 / 25     1        224     no  / no           4 / 7           128 / 64  2^11        2: the long step of the moving test)
    (256 200   25   6400   100 / 50 / 25     8        800     no  / yes          4 / 7           128 / 64  2^16        32: test_train_gpu.py, 200 / 100 tiles)
    405  200   25   10125  100 / 50 / 25     8        1280    no  / no           4 / 7           128 / 64  2^17        52
    40   2048  256  10240  1024 / 512 / 256  8        1280    no  / no           4 / 7           128 / 64  2^14        6

Both sides of every threshold the module claims are in the table.  K = 1 | 2 | 17 inside one 32-token granule (a K chunk whose
rows K .. 31 do not exist; kchunk 32, one split) | 33, one past it (kchunk 64, two splits of tn_dw_plan, the second with one
token).  S = 1 (a step that is the first and the last of both directions: h_prev = 0, softmax over one score) | 2 (a first and a
last with no middle one) | 3.  wp1 odd (5, 7, 11, 15) | even (4, 6, 8), wp2 odd (3, 5, 7) | even (2, 4), wp3 odd (1, 3) | even (2); at
T = 8 conv3's weight gradient is one strip of 8 tiles -- half a stage -- and the whole conv3 map one right edge.  Layer 1's
dx_splitk on at 6400 tokens (100 tiles, test_train_gpu.py) | off at 10125 and 10240 (ceil(K / 128) = 80 row tiles, 160 tiles: the
first count past its upper end, K > 10112; layer 0 has 320 there and left it at 5056 tokens).  Above 6400 tokens every split of
tn_dw_plan sums a longer token chunk into its one fp16-product accumulator set than any other test: 2560 / 1472 tokens of layer
0 / 1 against 1600 / 928 at 6400.  (405, 200) is 25 full groups of 16 clips and one of 5; (40, 2048) reaches the same threshold by
length: 256-step recurrences, three groups, the last of 8.

Training reference and bounds are train_step_ref._training_case's, unchanged: the float64 oracle differentiated at the device's
own z / y values; loss 2e-5, logits 5e-5, all 29 gradients and the five stage gradients of the workspace (divided by the loss
scale) max |a - b| <= 2e-3 * rms, norms within 1e-3 (+ 1e-7), BN running statistics rtol 1e-4, the input gradient
input_grad_ref.GRAD_BOUND.  Each case prints its figures before it asserts.  On top of them, at S = 1 the four weight_hh gradients
are dG^T . 0 (h_prev = 0) and must be exact zeros: a non-zero value would be a row that is not there.

Gradients that are zero in exact arithmetic (float64 oracle on the CPU: max |g| = 0): at S = 1 the four gru.weight_hh_* and
attention.weight / attention.bias (a softmax over one score is 1 whatever the score), at S >= 2 attention.bias alone.
_grad_errors compares such tensors absolutely; their norm bound is the absolute 1e-7 alone.  Every short case passes that same
1e-7 as ``norm_atol`` for the attention tensors that are zero at its S, which changes no bound and makes _training_case print
the device's, the float32 oracle's and the float64 oracle's norm of them (ATTN_ZERO_ATOL below, with what was measured: at S = 1
the device writes exact zeros for both, at S >= 2 at most 6.3e-9 for attention.bias).

Inference bounds are the neighbours': 2e-5 on init-scale weights and 2e-3 + identical argmax on cases.sharp_head
(test_model_gpu.py; float64 oracle margins of the sweep's clips: >= 2.7e-3 at init scale, >= 6.4e-2 under the sharp head, so the
argmax is decided), 2e-4 and the argmax wherever the oracle's top-2 margin is >= 1e-3 for the ragged call (test_ragged_infer_gpu.py;
every clip of the sweep is above it).  The ragged call holds every clip of the sweep at once, padded to 31 frames with NaN: the
pad-skip template utterance and the ragged right edges on conv3 maps of 2 to 7 columns (1 to 3 pooled ones).

Measured on an MI355X (loss err / logits err / worst gradient in rms / worst norm / worst stage gradient in rms; the float32 oracle's
own worst gradient against the float64 one is 1.1e-5 .. 2.4e-5 * rms at the short shapes):

    (1, 8)     2.9e-7  5.4e-8  1.5e-5  9.0e-8  3.1e-6   (dfeats 3.3e-6)      (17, 8)      7.2e-8  1.0e-7  1.1e-5  1.4e-7  4.1e-6
    (1, 9)     2.5e-8  6.5e-8  1.6e-5  8.6e-8  3.0e-6                        (33, 15)     1.5e-7  1.1e-7  1.3e-5  7.3e-7  4.3e-6
    (2, 10)    2.4e-7  7.1e-8  1.6e-5  3.8e-7  3.2e-6                        (3, 15) p=.5 1.4e-8  9.8e-8  2.0e-5  1.4e-7  4.2e-6
    (1, 12)    6.1e-8  4.5e-8  2.4e-5  1.2e-7  3.7e-6                        (8, 16) p=.5 1.6e-7  1.4e-7  1.6e-5  2.4e-7  3.8e-6
    (3, 15)    2.8e-7  8.2e-8  1.6e-5  2.2e-7  3.7e-6                        (405, 200)   9.1e-8  2.4e-7  3.0e-5  1.1e-6  6.1e-6
    (1, 16)    9.5e-8  9.1e-8  1.9e-5  1.2e-7  3.8e-6                        (40, 2048)   2.2e-7  3.9e-7  2.8e-5  1.8e-6  6.8e-6
    (2, 23)    2.5e-7  5.9e-8  1.6e-5  7.3e-8  3.5e-6   (dfeats 3.5e-6)
    (1, 31)    2.0e-7  8.5e-8  1.3e-5  2.2e-7  3.6e-6

The long splits hold: the worst gradient above 6400 tokens, 3.0e-5 * rms, is 1 / 60 of the bound and next to the short shapes' 2e-5.
Dense inference: at most 8.7e-8 at init scale and 3.6e-6 under the sharp head over the 26 cases; the ragged calls 8.7e-8.

CPU oracle times: well under a second for every short case; the two long cases print theirs (16 threads: host reproduction of
z / y 8 s and 10 s, float64 forward and backward 15 s and 35 s at (405, 200) and (40, 2048)), which is why their float32
comparison is off.  Both are the smallest shapes that cross the 160-tile threshold, by batch and by length."""
import ctypes as C
import os

import pytest
import torch

import cases
from oracle import model_ref
from sir_amd import _native, ops, synth, train_ops
from sir_amd.featurizer import get_featurizer
from sir_amd.models.models import CNNAudioGRU
from train_step_ref import _training_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
WEIGHT_HH = ["gru.weight_hh_l0", "gru.weight_hh_l0_reverse", "gru.weight_hh_l1", "gru.weight_hh_l1_reverse"]
# The absolute term of the norm bound of a gradient that is zero in exact arithmetic: _training_case's own 1e-7, passed by name so
# that the three norms are printed.  Measured (device / float32 oracle / float64 oracle): both attention tensors exactly 0 / 0 / 0 in
# every S = 1 case; attention.bias at S >= 2: (1, 16) 3.7e-9 / 7.5e-9 / 2.1e-17, (2, 23) 1.4e-9 / 4.7e-10 / 7.8e-18, (1, 31) 6.3e-9 /
# 1.2e-9 / 1.4e-17, (8, 16) with dropout 5.4e-9 / 0 / 3.5e-18.  No case comes near 1e-7: no bound is restated in this module.
ATTN_ZERO_ATOL = 1e-7
SHORT = [(1, 8), (1, 9), (2, 10), (1, 12), (3, 15), (1, 16), (2, 23), (1, 31), (17, 8), (33, 15)]
INFER_TS = list(range(8, 18)) + [23, 24, 31]
INFER_TMAX = 31
RAGGED_TOL, RAGGED_MARGIN = 2e-4, 1e-3
MOVE = ((1, 8), (8, 200), (1, 9), (8, 200), (1, 8))


def _f64(sd):
    return {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in sd.items()}


@pytest.fixture(scope="module")
def sd():
    return synth.synth_state_dict(31, seed=0)


@pytest.fixture(scope="module")
def sharp_sd(sd, model_golden):
    return cases.sharp_head(sd, model_golden["sharp_fc_bias"])


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


def _attn_zero(t):
    names = ["attention.bias"] + (["attention.weight"] if t // 8 == 1 else [])
    return {n: ATTN_ZERO_ATOL for n in names}


def _short_case(sd, bsz, t, **kw):
    print(f"T={t}:")
    m = _training_case(sd, bsz, t, norm_atol=_attn_zero(t), **kw)
    if t // 8 == 1:                                      # dG^T . 0: h_prev = 0 at the only step of either direction
        g = dict(m.named_parameters())
        for name in WEIGHT_HH:
            assert torch.count_nonzero(g[name].grad).item() == 0, name


# ---- short end: training at 1 to 33 tokens ----------------------------------------------------------------------------------
@pytest.mark.parametrize("bsz,t", SHORT)
def test_short_training_step_vs_oracle(sd, bsz, t):
    _short_case(sd, bsz, t)


@pytest.mark.parametrize("bsz,t", [(1, 8), (2, 23)])
def test_short_training_step_vs_oracle_with_input_gradient(sd, bsz, t):
    """``dfeats`` requested (sir_model_train_bwd_x) and compared with the oracle's x.grad at test_input_grad_gpu.py's bound"""
    _short_case(sd, bsz, t, want_dx=True)


@pytest.mark.parametrize("bsz,t", [(3, 15), (8, 16)])
def test_short_training_step_vs_oracle_with_dropout(sd, bsz, t):
    """The keep mask rebuilt on the host, checked bit for bit against y0d, fed to the oracle: 1536 and 8192 mask elements
    ((1, 8) has 512, which puts _training_case's keep-rate window (0.45, 0.55) only two sigma out: no dropout there).  The mask
    is the one of dropout step 4 whatever ran before this test in the process (the counter is put back afterwards): keep rates
    0.4967 and 0.4926."""
    step = train_ops.dropout_step()
    train_ops.set_dropout_step(4)
    try:
        _short_case(sd, bsz, t, dropout=0.5)
    finally:
        train_ops.set_dropout_step(step + 1)


# ---- the device against itself: bit identity ---------------------------------------------------------------------------------
def _step(m, x, y):
    for p in m.parameters():
        p.grad = None
    logits = m(x)
    loss = train_ops.fused_cross_entropy(logits, y)
    loss.backward()
    torch.cuda.synchronize()
    return logits.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters()}


def _batch(bsz, t):
    return cases.varied_features(bsz, t, seed=5000 + 8 * bsz + t).to(DEV), synth.synth_labels(bsz, 31, seed=bsz + t).to(DEV)


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


def test_short_backward_in_two_halves_is_bit_identical(sd, monkeypatch):
    """sir_model_train_bwd_part(HEAD_GRU) followed by (CNN) gives the bytes of sir_model_train_bwd at (1, 8) and (3, 15): the
    method of test_train_gpu.py::test_backward_in_two_halves_is_bit_identical (the data-parallel code path forced with a
    one-rank gloo group), and the same through direct C calls into a gradient buffer of their own."""
    import torch.distributed as dist
    lib, h = _native.lib(), get_featurizer().handle
    shapes = ((1, 8), (3, 15))
    ref = {}
    for bsz, t in shapes:
        x, y = _batch(bsz, t)
        _, ref[bsz, t] = _step(_train_model(sd), x, y)
        assert max(g.abs().max().item() for g in ref[bsz, t].values()) > 0
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29659")
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        monkeypatch.setattr(train_ops, "world_size", lambda: 2)          # take the two-bucket branch
        monkeypatch.setattr(train_ops, "OVERLAP_GRAD_EXCHANGE", True)
        for bsz, t in shapes:
            x, y = _batch(bsz, t)
            _, got = _step(_train_model(sd), x, y)
            for n, g in got.items():
                # sum over a 1-rank group = identity, then * 1/2 from the patched world size
                assert torch.equal(g * 2.0, ref[bsz, t][n]), (bsz, t, n)
    finally:
        dist.destroy_process_group()
        monkeypatch.undo()
    for bsz, t in shapes:
        x, y = _batch(bsz, t)
        m = _train_model(sd)
        logits = m(x)
        dlogits, loss = torch.empty_like(logits), torch.empty((), device=DEV)
        _native.check(lib.sir_ce_loss(h, logits.data_ptr(), y.data_ptr(), bsz, 31, loss.data_ptr(), dlogits.data_ptr(), 1.0,
                                      _native.current_stream_ptr()), "sir_ce_loss")
        whole = _c_backward(m, x, dlogits, [_native.BWD_ALL])
        halves = _c_backward(m, x, dlogits, [_native.BWD_HEAD_GRU, _native.BWD_CNN])
        assert torch.equal(whole, torch.cat([g.flatten() for g in ref[bsz, t].values()])), (bsz, t)
        assert torch.equal(halves, whole), (bsz, t)
    ops.check_status()


def _scribble(buf):
    """test_long_sequence_gpu.py's: float bit patterns whose top 16 bits are plausible forward-granule tags {7-bit epoch, 9-bit
    step + 1} -- steps 1..256 under each of the 128 epochs in turn -- then the prepared weights kept in the workspace are
    invalidated."""
    v = buf[: buf.numel() & ~3].view(torch.int32)
    i = torch.arange(v.numel(), device=buf.device, dtype=torch.int64)
    tag = (((i >> 8) & 127) << 9) | (i % 256 + 1)
    bits = (tag << 16) | 0x1234
    v.copy_(torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(torch.int32))
    ops.bump_weights_epoch()


def test_training_moving_between_one_token_and_two_hundred(sd):
    """One model object steps through (1, 8) -> (8, 200) -> (1, 9) -> (8, 200) -> (1, 8), its workspace (allocated for the
    largest shape up front) scribbled before every step: the logits and all 29 gradients of every step are bit-identical to
    the same step on a fresh model.  A one-token step reads nothing a 200-token step left behind, and the reverse."""
    batches = {key: _batch(*key) for key in set(MOVE)}
    fresh = {key: _step(_train_model(sd), *batches[key]) for key in batches}
    m = _train_model(sd)
    ops.cached_weights(m)
    ws = train_ops._train_state(m)["ws"]
    ws.get(_native.lib().sir_model_workspace_bytes(get_featurizer().handle, 8, 200, 1), torch.device(DEV, torch.cuda.current_device()))
    for step, key in enumerate(MOVE):
        m.load_state_dict(sd)                            # the same weights and BN buffers every time
        _scribble(m._sir_train["ws"].buf)
        logits, grads = _step(m, *batches[key])
        assert len(grads) == 29
        assert torch.equal(logits, fresh[key][0]), (step, key)
        for n, g in grads.items():
            assert g.isfinite().all(), (step, key, n)
            assert torch.equal(g, fresh[key][1][n]), (step, key, n)
    ops.check_status()


# ---- short end: inference at 8 to 31 frames ---------------------------------------------------------------------------------
def _margin(ref):
    top2 = ref.topk(2, dim=1).values
    return top2[:, 0] - top2[:, 1]


@pytest.fixture(scope="module")
def infer_data(sd, sharp_sd):
    """Three clips of 31 frames and the float64 oracle logits of their first t frames for every t of the sweep, computed once
    (0.3 s on the CPU).  In eval mode a row does not see its batch: a batch of B is the first B rows.  cases.sharp_head changes
    the classifier alone: its logits are that classifier on the oracle's context vectors."""
    x = cases.varied_features(3, INFER_TMAX, seed=831).float()
    sd64, sharp64 = _f64(sd), _f64(sharp_sd)
    for k in sd64:
        assert k in ("fc.weight", "fc.bias") or torch.equal(sd64[k], sharp64[k]), k
    ref, ref_sharp = {}, {}
    with torch.no_grad():
        for t in INFER_TS:
            st = {}
            ref[t] = model_ref.forward(sd64, x[:, :, :t].double(), stages=st)
            ref_sharp[t] = st["ctx"] @ sharp64["fc.weight"].t() + sharp64["fc.bias"]
    return {"x": x, "ref": ref, "ref_sharp": ref_sharp}


@pytest.mark.parametrize("bsz", [1, 3])
@pytest.mark.parametrize("t", INFER_TS)
def test_short_dense_inference_vs_oracle(sd, sharp_sd, infer_data, t, bsz):
    x = infer_data["x"][:bsz, :, :t].contiguous().to(DEV)
    ref, ref_sharp = infer_data["ref"][t][:bsz], infer_data["ref_sharp"][t][:bsz]
    lg, am = _eval_model(sd).predict(x)
    lgs, ams = _eval_model(sharp_sd).predict(x)
    torch.cuda.synchronize()
    err = (lg.cpu().double() - ref).abs().max().item()
    errs = (lgs.cpu().double() - ref_sharp).abs().max().item()
    print(f"T={t} B={bsz} dense: max |logit error| {err:.2e} (init scale; smallest oracle margin {_margin(ref).min().item():.2e}), "
          f"{errs:.2e} (sharp head; smallest oracle margin {_margin(ref_sharp).min().item():.2e})")
    assert _margin(ref).min().item() > 2 * 2e-5 and _margin(ref_sharp).min().item() > 2 * 2e-3      # the argmax is decided
    assert err <= 2e-5
    assert torch.equal(am.cpu(), lg.cpu().argmax(1)) and torch.equal(am.cpu(), ref.argmax(1))
    assert errs < 2e-3
    assert torch.equal(ams.cpu(), ref_sharp.argmax(1))
    ops.check_status()


@pytest.mark.parametrize("bsz", [1, 3])
def test_short_ragged_inference_vs_oracle(sd, infer_data, bsz):
    """The clips of the dense sweep as ONE ragged call: 13 x bsz rows padded to 31 frames with NaN, ``lengths`` = the sweep, on a
    0xFF-filled workspace; every reference row is the clip alone at its own length."""
    rows = [(t, b) for t in INFER_TS for b in range(bsz)]
    n = len(rows)
    x = torch.full((n, 64, INFER_TMAX), float("nan"))
    for i, (t, b) in enumerate(rows):
        x[i, :, :t] = infer_data["x"][b, :, :t]
    ref = torch.stack([infer_data["ref"][t][b] for t, b in rows])
    ws = ops.Workspace()
    ws.get(_native.lib().sir_model_workspace_bytes(get_featurizer().handle, n, INFER_TMAX, 0), torch.device(DEV, torch.cuda.current_device())).fill_(0xFF)
    lg, am = ops.model_infer(_eval_model(sd), x.to(DEV), ws, want_argmax=True,
                             lengths=torch.tensor([t for t, _ in rows], dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    lg, am = lg.cpu(), am.cpu()
    assert not lg.isnan().any()
    err = (lg.double() - ref).abs().max().item()
    clear = _margin(ref) >= RAGGED_MARGIN
    print(f"T=8..31 B={n} ragged: max |logit error| {err:.2e}, {int((~clear).sum())} clips below the argmax margin "
          f"(smallest oracle margin {_margin(ref).min().item():.2e})")
    assert err <= RAGGED_TOL
    assert torch.equal(am[clear], ref.argmax(1)[clear])
    assert int(clear.sum()) >= n // 2
    ops.check_status()


# ---- long end: training above 6400 tokens -----------------------------------------------------------------------------------
def test_training_step_vs_oracle_405x200(sd):
    """K = 10125: ceil(K / 128) = 80 row tiles, 160 layer-1 tiles -- the first shape past dx_splitk's upper end, both layers'
    input gradients in one pass; 25 full groups of 16 clips and one of 5; tn_dw_plan's splits 2560 / 1472 tokens long."""
    print("T=200:")
    _training_case(sd, 405, 200, compare_f32=False, oracle_time=True)


def test_training_step_vs_oracle_40x2048(sd):
    """K = 10240: the same threshold reached by length -- 256-step recurrences, loss scale 2^14, three groups (16, 16, 8)."""
    print("T=2048:")
    _training_case(sd, 40, 2048, compare_f32=False, oracle_time=True)
