"""Batches above 256 against the oracle: half chip (B <= 256), full chip (B = 512) and beyond (oversubscribed: the GRU
recurrences launch 8 * ceil(B / 16) workgroups, one per CU, and rest on in-order dispatch past 256 of them).

Every shape is t = 24 frames: wp1 = 12, wp2 = 6 (Winograd right-edge tiles), S = 3 GRU steps (a first, a middle, a last).
The module is ordered by regime -- the loss kernel alone, then everything up to the full chip, then the oversubscribed
batches, then the sequences that move between batch sizes -- so that B = 512 has run before anything oversubscribed.

What each batch lands on (csrc/train_workspace.h, wgrad_wino_f16x3_kernel.h, wino2_geo.h, gru_quad.hip; 256 CUs).  K = B * S
tokens; ksplits 1 / 2 / 8 below 256 / below 2048 / from 2048 tokens; dx_splitk (the layer-input gradient as two K halves) for
48 <= tiles < 160, tiles = ceil(K / 128) * in / 256; nsplit = K splits of tn_dw_plan; strips = wgrad_wino_strips of conv2 /
conv3 (caps 128 / 64); stat = Winograd spatial tasks of conv2 / conv3 before wino2_stat_blocks caps them at the CU count;
map = block-to-cluster map of the recurrences (x8: the multiple-of-8 form, plain otherwise).

    B     K     ksplits  dx_splitk l0 / l1  nsplit l0 / l1  strips   stat tasks      loss scale  clusters  map    workgroups
    8     24    1        no  / no           1 / 1           48 / 8   24 / 6          2^11        2         plain  8
    16    48    1        no  / no           2 / 2           96 / 24  48 / 12         2^12        2         plain  8
    257   771   2        no  / no           4 / 7           128 / 64 772* / 193      2^17        34        plain  136
    512   1536  2        yes / no           4 / 7           128 / 64 1536* / 384*    2^17        64        x8     256 (= CUs)
    528   1584  2        yes / no           4 / 7           128 / 64 1584* / 396*    2^18        66        plain  264
    1024  3072  8        yes / yes          4 / 7           128 / 64 3072* / 768*    2^18        128       x8     512
    1041  3123  8        yes / yes          4 / 7           128 / 64 3124* / 781*    2^19        132       plain  528
    (256 at t = 200, test_train_gpu.py: K = 6400, ksplits 8, dx_splitk no / yes, 4 / 7, 128 / 64, capped, 2^16, 32, x8, 128)
    * capped at the CU count.

Both sides of every threshold a batch <= 1100 reaches at t = 24 are in the table: ksplits 2 | 8 (1 at B = 8 / 16),
dx_splitk of layer 0 off (257) | on (512 ...) and of layer 1 off (... 528) | on (1024, 1041), conv3's statistics blocks
uncapped (257) | capped, nsplit and the strips below their caps at B = 8 / 16 and at them above.  dx_splitk's upper
ends (160 tiles: B >= 1665 / 3329) lie beyond 1100 (test_token_range_gpu.py crosses them at t = 200 and t = 2048).  Inference runs B = 512, 528, 1024, 1041; training 257, 512, 528, 1041.
ce_loss_kernel's second trip needs B > 256, fc_wgrad_block's second chunk B > 1024 (1041 = 1024 + 2 * 8 + 1: the unrolled
body and the scalar tail behind it).

Training reference: the method of test_train_gpu.py::test_training_step_at_bench_batch_256_vs_oracle -- the float64 oracle
differentiated at the device's own z / y values (train_step_ref.py; _views is not tied to t = 200), with that test's bounds
unchanged: loss 2e-5, logits 5e-5, all 29 gradients max|a - b| <= 2e-3 * rms, norms within 1e-3, BN running statistics
rtol 1e-4.  The intermediate gradients in the workspace divided by the loss scale (dy1, dy0, dx0, da2, da1) are held to
the same 2e-3 * rms (test_train_forward_backward_stages' bound): the parameter gradients alone cannot see a wrong loss
scale, which is multiplied in and out again.  Each case prints, before it asserts, the float32 oracle's own distance from
the float64 oracle at the same forward values next to the device's; no bound was widened.

CPU oracle times (8 threads): the float64 training oracle takes 1.8 s at B = 257, 1.6 s at B = 528 and 3.4 s at B = 1041
(float32: 1.6 s; the eval-mode forward of all 1041 rows 0.6 s), so no case drops to t = 16.  The inference references are
computed once for 1041 rows and sliced: in eval mode a row does not see its batch.

Inference bounds are the neighbours': 2e-5 on init-scale weights and 2e-3 + identical argmax on cases.sharp_head
(test_model_gpu.py), bit-identity of +0.0 against -0.0 tails (test_pad_skip_gpu.py), 2e-4 and the argmax wherever the
oracle's top-2 margin is >= 1e-3 for the ragged call (test_ragged_infer_gpu.py; its reference rows are model_ref.forward on
the clips of one length together, which in eval mode is the clip alone)."""
import ctypes as C

import pytest
import torch

import cases
import recipe_ref
from oracle import model_ref
from sir_amd import _native, ops, synth, train_ops
from sir_amd.featurizer import get_featurizer
from sir_amd.models.models import CNNAudioGRU
from train_step_ref import _training_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = 24
S = 3
NMAX = 1041
U = 2.0 ** -24
RAGGED_TOL, RAGGED_MARGIN = 2e-4, 1e-3
TAILS = [1, 3, 7, 9, 10, 12, 17, 20, 23]                 # data extents of the rows with a +0.0 tail: 1, 2 and 3 live GRU steps


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


def _frames(n):
    return [8 + (7 * i) % 17 for i in range(n)]          # mixed over [8, 24]


@pytest.fixture(scope="module")
def data(sd, sharp_sd):
    """1041 clips and their oracle logits, computed once; a batch of B is the first B rows."""
    x = cases.varied_features(NMAX, T, seed=2024).float()
    xz = x.clone()                                       # about a third of the rows: +0.0 tails of different lengths
    for i in range(1, NMAX, 3):
        xz[i, :, TAILS[(i // 3) % len(TAILS)]:] = 0.0
    frames = _frames(NMAX)
    xn = x.clone()
    for b, f in enumerate(frames):
        xn[b, :, f:] = float("nan")
    with torch.no_grad():
        ref = model_ref.forward(sd, x)
        ref_sharp = model_ref.forward(sharp_sd, x)
        ref_tails = model_ref.forward(sd, xz)
        ref_ragged = torch.empty(NMAX, 31)
        for f in sorted(set(frames)):
            rows = [b for b, fb in enumerate(frames) if fb == f]
            ref_ragged[rows] = model_ref.forward(sd, x[rows][:, :, :f].contiguous())
    return {"x": x, "xz": xz, "xn": xn, "frames": frames, "ref": ref, "ref_sharp": ref_sharp, "ref_tails": ref_tails,
            "ref_ragged": ref_ragged}


def _infer(m, x, ws=None, **kw):
    lg, am = ops.model_infer(m, x, ws if ws is not None else ops.Workspace(), want_argmax=True, **kw)
    torch.cuda.synchronize()
    return lg, am


def _neg_tail(x):
    """the same features with the all-+0.0 tail of every utterance replaced by -0.0 (forces the full path)"""
    nz = (x.view(torch.int32) != 0).any(dim=1)
    e0 = (nz * (torch.arange(x.shape[2], device=x.device) + 1)).amax(dim=1)
    tail = (torch.arange(x.shape[2], device=x.device)[None, None, :] >= e0[:, None, None]).expand_as(x)
    return torch.where(tail, torch.full_like(x, -0.0), x)


def _scribble(buf):
    """test_robustness_gpu.py's: float bit patterns whose top 16 bits are plausible forward-granule tags, then the prepared
    weights kept in the workspace are invalidated."""
    v = buf.view(torch.int32)
    steps = torch.arange(v.numel(), device=buf.device, dtype=torch.int32) % 25 + 1
    v.copy_(((0x3E00 + steps) << 16) | 0x1234)
    ops.bump_weights_epoch()


# ---- the loss kernel alone (one workgroup striding over the rows: no recurrence) ------------------------------------------
def _loss_case(bsz, ncls, second, seed):
    """test_recipe_gpu.py's case: two ignored rows (2 and B - 1), the second label of an ignored row invalid"""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(bsz, ncls, generator=g) * 3.0
    ya = torch.randint(0, ncls, (bsz,), generator=g)
    yb = lam = None
    if second:
        yb = torch.randint(0, ncls, (bsz,), generator=g)
        lam = torch.rand(bsz, generator=g)
        lam[0], lam[1], lam[bsz - 2] = 0.0, 1.0, 0.0
        yb[3] = ya[3]
    ya[2] = -100
    ya[bsz - 1] = -100
    if second:
        yb[2] = 10 ** 6
    return logits, ya, yb, lam


def _dev(t):
    return None if t is None else t.to(DEV)


@pytest.mark.parametrize("bsz", [257, 512, 1041])
@pytest.mark.parametrize("ncls", [6, 31])
@pytest.mark.parametrize("eps,second", [(0.0, False), (0.1, True)])
def test_loss_and_gradient_vs_float64(bsz, ncls, eps, second):
    """sir_ce_loss (eps 0, one label) and sir_ce_loss_soft (smoothing + mixup's second label) with rows behind the first trip
    of the 256-row stride; the bounds of test_recipe_gpu.py::test_soft_loss_and_gradient_vs_float64: loss 1e-5,
    dlogits (C + 8 + R) * 2^-24 / n_valid per element."""
    logits, ya, yb, lam = _loss_case(bsz, ncls, second, seed=17 * bsz + ncls)
    lg = logits.to(DEV).requires_grad_(True)
    loss = train_ops.fused_cross_entropy(lg, _dev(ya), _dev(yb), _dev(lam), label_smoothing=eps)
    loss.backward()
    ref_loss, ref_d = recipe_ref.soft_ce(logits, ya, yb, lam, eps)
    n_valid = int((ya != -100).sum())
    err = abs(loss.item() - ref_loss.item())
    spread = (logits.max(dim=1).values - logits.min(dim=1).values).double()[:, None]
    bound = (ncls + 8 + spread) * U / n_valid
    derr = (lg.grad.cpu().double() - ref_d).abs()
    print(f"CE B={bsz} C={ncls} eps={eps} second={second}: |loss - ref| {err:.3e}, max dlogits err / bound {(derr / bound).max().item():.3f}")
    assert err <= 1e-5
    assert (derr <= bound).all()
    assert (lg.grad[ya.to(DEV) == -100] == 0).all()
    ops.check_status()


@pytest.mark.parametrize("bsz", [257, 512, 1041])
@pytest.mark.parametrize("ncls", [6, 31])
def test_loss_ignored_and_bad_labels_behind_row_256(bsz, ncls):
    """-100 only in rows >= 256: the divisor and the zero rows follow torch.  Then one label outside [0, C) in a row >= 256:
    NaN loss and SIR_EINVAL at the next check.  The hard-target soft call stays bit-identical to sir_ce_loss."""
    lib, h = _native.lib(), get_featurizer().handle
    g = torch.Generator().manual_seed(29 * bsz + ncls)
    logits = torch.randn(bsz, ncls, generator=g) * 3.0
    y = torch.randint(0, ncls, (bsz,), generator=g)
    ign = sorted({bsz - 1} | set(range(256, bsz - 2, 97)))
    y[ign] = -100
    a = logits.clone().to(DEV).requires_grad_(True)
    b = logits.clone().double().requires_grad_(True)
    la = train_ops.fused_cross_entropy(a, y.to(DEV))
    lb = torch.nn.functional.cross_entropy(b, y)
    la.backward()
    lb.backward()
    n_valid = bsz - len(ign)
    spread = (logits.max(dim=1).values - logits.min(dim=1).values).double()[:, None]
    assert abs(la.item() - lb.item()) <= 1e-5
    assert ((a.grad.cpu().double() - b.grad).abs() <= (ncls + 8 + spread) * U / n_valid).all()
    assert (a.grad[ign] == 0).all() and (a.grad[:256] != 0).all()
    ops.check_status()                                   # -100 is not an error
    # hard targets through the soft entry: the same launch, bit for bit
    lg, yd = logits.to(DEV), y.to(DEV)
    out = []
    for soft in (False, True):
        loss = torch.full((1,), -1.0, device=DEV)
        d = torch.full_like(lg, -1.0)
        if soft:
            rc = lib.sir_ce_loss_soft(h, lg.data_ptr(), yd.data_ptr(), None, None, 0.0, bsz, ncls, loss.data_ptr(), d.data_ptr(), 3.0,
                                      _native.current_stream_ptr())
        else:
            rc = lib.sir_ce_loss(h, lg.data_ptr(), yd.data_ptr(), bsz, ncls, loss.data_ptr(), d.data_ptr(), 3.0, _native.current_stream_ptr())
        _native.check(rc, "ce")
        out.append((loss, d))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert abs(out[0][0].item() - lb.item()) <= 1e-5
    # one bad label, in the last row of the second trip
    bad = y.clone()
    row = max(256, bsz - 2)
    bad[row] = ncls
    for soft_kw in ({}, {"label_smoothing": 0.1}):
        loss = train_ops.fused_cross_entropy(lg, bad.to(DEV), **soft_kw)
        torch.cuda.synchronize()
        assert torch.isnan(loss).item()
        with pytest.raises(_native.SirError, match="code -1"):
            ops.check_status()
        ops.check_status()                               # cleared by the failing check


# ---- inference against the oracle ---------------------------------------------------------------------------------------
def _position_rows(bsz):
    return [0, 255, 256, 511, bsz - 1] + ([1023, 1024, 1040] if bsz == NMAX else [])


def _inference_case(check, bsz, sd, sharp_sd, data):
    if check == "dense":
        x = data["x"][:bsz].to(DEV)
        lg, am = _infer(_eval_model(sd), x)
        err = (lg.cpu() - data["ref"][:bsz]).abs().max().item()
        lgs, ams = _infer(_eval_model(sharp_sd), x)
        errs = (lgs.cpu() - data["ref_sharp"][:bsz]).abs().max().item()
        top2 = data["ref_sharp"][:bsz].topk(2, dim=1).values
        print(f"B={bsz} dense: max |logit error| {err:.2e} (init scale), {errs:.2e} (sharp head; smallest oracle margin "
              f"{(top2[:, 0] - top2[:, 1]).min().item():.2e})")
        assert err <= 2e-5
        assert torch.equal(am.cpu(), lg.cpu().argmax(1))
        assert errs < 2e-3
        assert torch.equal(ams.cpu(), data["ref_sharp"][:bsz].argmax(1))
    elif check == "tails":
        m = _eval_model(sd)
        x = data["xz"][:bsz].to(DEV)
        xf = _neg_tail(x)
        assert not torch.equal(x.view(torch.int32), xf.view(torch.int32))
        ws = ops.Workspace()
        ws.get(_native.lib().sir_model_workspace_bytes(get_featurizer().handle, bsz, T, 0), x.device).fill_(0xFF)
        lg, am = _infer(m, x, ws)
        lgf, amf = _infer(m, xf)
        d3 = ops.pad_skip_tables(ws.buf, bsz, T)["d3"].tolist()
        assert {1, 2, 3} <= set(d3[:bsz]) and d3[bsz] == S        # the skip really ran, with every step count, and the template is whole
        assert torch.equal(lg.view(torch.int32), lgf.view(torch.int32)) and torch.equal(am, amf)
        err = (lg.cpu() - data["ref_tails"][:bsz]).abs().max().item()
        print(f"B={bsz} +0.0 tails: bit-identical to -0.0 tails, max |logit error| {err:.2e}")
        assert err <= 2e-5
    elif check == "ragged":
        m = _eval_model(sd)
        frames = data["frames"][:bsz]
        x = data["xn"][:bsz].to(DEV)
        ws = ops.Workspace()
        ws.get(_native.lib().sir_model_workspace_bytes(get_featurizer().handle, bsz, T, 0), x.device).fill_(0xFF)
        lg, am = _infer(m, x, ws, lengths=torch.tensor(frames, dtype=torch.int32, device=DEV))
        lg, am, ref = lg.cpu(), am.cpu(), data["ref_ragged"][:bsz]
        assert not lg.isnan().any()
        err = (lg - ref).abs().max().item()
        top2 = ref.topk(2, dim=1).values
        clear = (top2[:, 0] - top2[:, 1]) >= RAGGED_MARGIN
        print(f"B={bsz} ragged: max |logit error| {err:.2e}, {int((~clear).sum())} clips below the argmax margin")
        assert err <= RAGGED_TOL
        assert torch.equal(am[clear], ref.argmax(1)[clear])
        assert int(clear.sum()) >= bsz // 2
    else:
        assert check == "position"
        rows = _position_rows(bsz)
        m = _eval_model(sd)
        for key in ("x", "xz"):
            x = data[key][:bsz].to(DEV)
            lg, am = _infer(m, x)
            lgr, amr = _infer(m, x[rows].contiguous())
            assert torch.equal(lgr.view(torch.int32), lg[rows].view(torch.int32)) and torch.equal(amr, am[rows]), key
    ops.check_status()


CHECKS = ("dense", "tails", "ragged", "position")


# ---- up to the full chip: B = 257 (136 workgroups), B = 512 (256 workgroups = every CU) ------------------------------------
def _c_backward(m, x, dlogits, parts):
    """Direct C calls of the backward (one per entry of ``parts``) on the workspace ``m``'s last forward left, all 29
    gradients into a buffer of its own."""
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


@pytest.mark.parametrize("bsz", [257, 512])
def test_training_step_vs_oracle_up_to_full_chip(sd, bsz):
    _training_case(sd, bsz, T)


@pytest.mark.parametrize("check", CHECKS)
def test_inference_vs_oracle_full_chip(sd, sharp_sd, data, check):
    _inference_case(check, 512, sd, sharp_sd, data)


def test_two_full_chip_batches_in_flight(sd):
    """Four B = 512 batches through the library's two-slot pipeline from one caller stream (the method of
    test_model_gpu.py::test_library_pipeline_from_one_caller_stream): two cluster launches that each fill the chip, on
    different streams, chained by sir_cluster_enter.  Bit-identical to the single-stream results."""
    from sir_amd.pipeline import BatchPipeline
    m = _eval_model(sd)
    fz = get_featurizer()
    bsz, n = 512, 2
    waves = [synth.synth_clips(bsz, 10000 + 500 * i, seed=700 + i).to(DEV) for i in range(4)]
    lens = [(torch.arange(bsz, dtype=torch.int32) * 37 % 6000 + w.shape[1] - 6000).to(DEV) for w in waves]    # 8 .. 23 frames of data
    ref = []
    for w, l in zip(waves, lens):
        f = fz(w, l, t_pad=T).clone()
        ref.append((f, *m.predict(f)))
    torch.cuda.synchronize()
    pipe = BatchPipeline(m, n_streams=n)
    bufs = [torch.empty(bsz, 64, T, device=DEV) for _ in range(n)]
    acc = torch.zeros(bsz, 31, device=DEV)
    res = []
    for i, (w, l) in enumerate(zip(waves, lens)):
        k = pipe.slot(i)
        f = pipe.features(i, w, l, t_pad=T, out=bufs[k])
        res.append(pipe.infer(i, f))
    pipe.join()
    for logits, _ in res:
        acc += logits
    torch.cuda.synchronize()
    for (f0, l0, a0), (l1, a1) in zip(ref, res):
        assert torch.equal(l0, l1) and torch.equal(a0, a1)
    assert torch.equal(acc, sum(l for _, l, _ in ref))
    with torch.no_grad():
        oracle = model_ref.forward(sd, ref[0][0].cpu())
    assert (res[0][0].cpu() - oracle).abs().max().item() <= 2e-5
    ops.check_status()


# ---- oversubscribed: more workgroups than CUs, the recurrences rest on in-order dispatch ---------------------------------
@pytest.mark.parametrize("bsz,check", [(b, c) for b in (528, 1024, NMAX) for c in CHECKS])
def test_inference_vs_oracle_oversubscribed(sd, sharp_sd, data, bsz, check):
    _inference_case(check, bsz, sd, sharp_sd, data)


def test_training_step_vs_oracle_528_with_input_gradient(sd):
    """B = 528 (264 workgroups: the first oversubscription) with ``dfeats`` requested (sir_model_train_bwd_x) and compared with
    the oracle's x.grad at test_input_grad_gpu.py's bound, next to everything the other batches check."""
    _training_case(sd, 528, T, want_dx=True)


def test_training_step_vs_oracle_1041(sd):
    _training_case(sd, NMAX, T)


def test_training_step_vs_oracle_1041_with_dropout(sd):
    """The method of test_train_gpu.py::test_dropout_on_training_step_vs_oracle: the mask rebuilt on the host, checked bit for
    bit against what the dropout kernel wrote, fed to the oracle."""
    _training_case(sd, NMAX, T, dropout=0.5)


def test_backward_forms_are_bit_identical_at_528(sd):
    """The two-halves backward (SIR_BWD_HEAD_GRU + SIR_BWD_CNN) and the one-stream backward (every kernel timed:
    sir_profile_enable mode 1) against the default two-stream one: all 29 gradients bit-identical."""
    lib, h = _native.lib(), get_featurizer().handle
    bsz = 528
    x = cases.varied_features(bsz, T, seed=4000).to(DEV)
    y = synth.synth_labels(bsz, 31, seed=4001).to(DEV)
    m = _train_model(sd)

    def grads():
        m.zero_grad(set_to_none=True)
        loss = train_ops.fused_cross_entropy(m(x), y)
        loss.backward()
        torch.cuda.synchronize()
        return torch.cat([p.grad.flatten() for p in m.parameters()]).clone()

    two = [grads() for _ in range(2)]
    assert two[0].abs().max() > 0 and torch.equal(two[0], two[1])
    _native.check(lib.sir_profile_enable(h, 1, -1), "sir_profile_enable")
    try:
        one = grads()
    finally:
        nk = lib.sir_profile_kernel_count()
        ms, cnt = (C.c_double * nk)(), (C.c_int64 * nk)()
        lib.sir_profile_collect(h, ms, cnt, nk)
        _native.check(lib.sir_profile_enable(h, 0, -1), "sir_profile_enable")
    assert torch.equal(one, two[0])
    logits = m(x)                                        # (the running statistics move; the batch statistics and gradients do not)
    dlogits, loss = torch.empty_like(logits), torch.empty((), device=DEV)
    _native.check(lib.sir_ce_loss(h, logits.data_ptr(), y.data_ptr(), bsz, 31, loss.data_ptr(), dlogits.data_ptr(), 1.0,
                                  _native.current_stream_ptr()), "sir_ce_loss")
    whole = _c_backward(m, x, dlogits, [_native.BWD_ALL])
    halves = _c_backward(m, x, dlogits, [_native.BWD_HEAD_GRU, _native.BWD_CNN])
    assert torch.equal(whole, two[0])
    assert torch.equal(halves, whole)
    ops.check_status()


# ---- moving between small and large batches on one handle: the exchange buffers grow and are zeroed again -----------------
def test_inference_moving_between_small_and_large_batches(sd, data):
    m = _eval_model(sd)
    first = {}
    for step, bsz in enumerate((16, NMAX, 16, 512, NMAX)):
        lg, am = m.predict(data["xz"][:bsz].to(DEV))
        torch.cuda.synchronize()
        if bsz not in first:
            first[bsz] = (lg.clone(), am.clone())
        assert torch.equal(lg, first[bsz][0]) and torch.equal(am, first[bsz][1]), (step, bsz)
        if step >= 1:
            _scribble(m._ws.buf)
    for bsz, (lg0, am0) in first.items():                # and what a fresh module on a fresh workspace gives
        lg, am = _infer(_eval_model(sd), data["xz"][:bsz].to(DEV))
        assert torch.equal(lg, lg0) and torch.equal(am, am0), bsz
    assert (first[NMAX][0].cpu() - data["ref_tails"]).abs().max().item() <= 2e-5
    ops.check_status()


def test_training_moving_between_small_and_large_batches(sd):
    m = _train_model(sd)
    batches = {b: (cases.varied_features(b, T, seed=5000 + b).to(DEV), synth.synth_labels(b, 31, seed=b).to(DEV)) for b in (8, 528)}
    first = {}
    for step, bsz in enumerate((8, 528, 8, 528)):
        x, y = batches[bsz]
        for p in m.parameters():
            p.grad = None
        m.load_state_dict(sd)                            # the same weights and BN buffers every time
        loss = train_ops.fused_cross_entropy(m(x), y)
        loss.backward()
        torch.cuda.synchronize()
        g = torch.cat([p.grad.flatten() for p in m.parameters()]).clone()
        if bsz not in first:
            first[bsz] = (loss.detach().clone(), g)
        assert torch.equal(loss.detach(), first[bsz][0]), (step, bsz)
        assert torch.equal(g, first[bsz][1]), (step, bsz)
        if step >= 1:
            _scribble(m._sir_train["ws"].buf)
    ops.check_status()
