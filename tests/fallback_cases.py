"""The cases of ``test_conv_fallback_gpu.py``: what one child process runs on the fallback conv kernels (``SIR_CONV_FALLBACK`` is read
once per process, so every group below runs in a process of its own: ``python -c``-style script -> ``main(group)``).  Each case prints
one line with the figures it measured before it asserts; a group ends with the token ``FALLBACK-CASES-OK <group>`` and its wall time.

References and bounds are the suite's own, unchanged: ``train_step_ref._training_case`` (float64 oracle at the device's ReLU / max-pool
values; loss 2e-5, logits 5e-5, gradients and stage gradients 2e-3 * rms, norms 1e-3), ``input_grad_ref`` (2e-3 * rms), the inference
bounds of ``test_token_range_gpu.py`` (2e-5 at init scale, 2e-3 under the sharp head, 2e-4 ragged, argmax where the margin decides) and
``range_ref`` for the operand-range cases.  bf16x6 products are specified as fp32-accurate: the fallback kernels get no bound of their own."""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

import cases
import input_grad_ref
import range_ref
from oracle import model_ref
from sir_amd import _native, ops, synth, train_ops
from sir_amd.featurizer import get_featurizer
from sir_amd.models.models import CNNAudioGRU
from train_step_ref import _device_forward_values, _oracle_f64, _rel, _views

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (batch, t_frames, want_dx) -- t chosen for the fallback kernels' own tiling (module docstring of test_conv_fallback_gpu.py)
TRAIN_SHORT = [(1, 8, False), (2, 9, True), (3, 10, False), (1, 12, False), (2, 14, False), (3, 15, True), (2, 23, False), (1, 31, False),
               (17, 8, False), (33, 15, False)]
TRAIN_TILES = [(3, 36, False), (2, 60, False), (1, 64, False), (3, 68, True), (2, 130, False), (1, 256, False), (2, 257, True)]
DROPOUT_CASE = (3, 36)
VARIANT_SHAPES = [(3, 68), (2, 257)]
REFUSED = [(1, 258), (1, 260), (2, 520)]
NATURAL = (2048, 256)
INFER_BATCHES = (1, 5)
SENTINEL = 0x7FC12345                                    # a NaN bit pattern no kernel writes
PAD_LENGTHS = [700, 2500, 4200, 6000, 8000, 10000, 12300, 48000, 0, 3000, 144000]     # samples: extents from 2 frames to the full width


def _f64(sd):
    return {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in sd.items()}


def _sd():
    return synth.synth_state_dict(31, seed=0)


def _model(sd, train, frozen_bn=()):
    m = CNNAudioGRU(31)
    m.load_state_dict(sd)
    m = m.to(DEV)
    m.train(train)
    m.gru.dropout = 0.0
    for i in frozen_bn:
        getattr(m, f"bn{i}").eval()
    return m


def _inputs(bsz, t):
    """the inputs of ``train_step_ref._training_case`` at this shape"""
    return cases.varied_features(bsz, t, seed=3000 + bsz), synth.synth_labels(bsz, 31, seed=3001 + bsz)


# ---- training step against the float64 oracle --------------------------------------------------------------------------------
def _train_cases(sd, shapes):
    from test_token_range_gpu import _short_case
    for bsz, t, want_dx in shapes:
        out = {}
        t0 = time.perf_counter()
        _short_case(sd, bsz, t, want_dx=want_dx, out=out)
        dx = f" dfeats {out['dx']:.1e}" if want_dx else ""
        print(f"CASE train B={bsz} T={t}: loss {out['loss']:.1e} logits {out['logits']:.1e} grad {out['grad']:.1e} norm {out['norm']:.1e} "
              f"stage {out['stage']:.1e}{dx} ({time.perf_counter() - t0:.1f} s)")


def group_train_short():
    _train_cases(_sd(), TRAIN_SHORT)


def group_train_tiles():
    from test_token_range_gpu import _short_case
    sd = _sd()
    _train_cases(sd, TRAIN_TILES)
    bsz, t = DROPOUT_CASE
    train_ops.set_dropout_step(4)                        # the mask of dropout step 4, as in test_token_range_gpu.py
    out = {}
    _short_case(sd, bsz, t, dropout=0.5, out=out)
    print(f"CASE train B={bsz} T={t} p=.5: loss {out['loss']:.1e} logits {out['logits']:.1e} grad {out['grad']:.1e} norm {out['norm']:.1e} "
          f"stage {out['stage']:.1e}")


# ---- direct C calls of the backward ------------------------------------------------------------------------------------------
class _Fwd:
    """One training-mode forward of ``sd`` at (bsz, t) on the device, kept: the C backward may be called on it many times."""

    def __init__(self, sd, bsz, t, frozen_bn=()):
        self.sd, self.bsz, self.t = sd, bsz, t
        self.x, self.y = _inputs(bsz, t)
        self.m = _model(sd, True, frozen_bn)
        self.xd = self.x.to(DEV)
        self.logits = self.m(self.xd).detach()
        lib, h = _native.lib(), get_featurizer().handle
        self.dlogits, self.loss = torch.empty_like(self.logits), torch.empty((), device=DEV)
        _native.check(lib.sir_ce_loss(h, self.logits.data_ptr(), self.y.to(DEV).data_ptr(), bsz, 31, self.loss.data_ptr(),
                                      self.dlogits.data_ptr(), 1.0, _native.current_stream_ptr()), "sir_ce_loss")
        torch.cuda.synchronize()
        self.ws = self.m._sir_train["ws"].buf
        self.names = [n for n, _ in self.m.named_parameters()]

    def oracle_values(self):
        return _device_forward_values(self.m, self.sd, self.x, self.bsz, self.t, _views(self.m, self.bsz, self.t))

    def call(self, fn, part=_native.BWD_ALL, buf=None, null=(), dfeats=None):
        """One C call of backward entry point ``fn`` into ``buf`` (a fresh zeroed GradBuffer by default), gradient pointers of the
        parameters named in ``null`` NULL -> (return code, buffer)."""
        lib, h = _native.lib(), get_featurizer().handle
        buf = buf if buf is not None else train_ops.GradBuffer(self.m)
        g, _ = buf.struct_for(tuple(n not in null for n in self.names))
        w, _keep = ops.cached_weights(self.m)
        seed, p = self.m._sir_last_dropout
        head = [h, C.byref(w), self.xd.data_ptr(), self.dlogits.data_ptr(), self.bsz, self.t, p, seed]
        tail = [self.ws.data_ptr(), self.ws.numel()]
        st = _native.current_stream_ptr()
        cfg = C.byref(train_ops.bn_config(self.m))
        if fn == "sir_model_train_bwd":
            assert part == _native.BWD_ALL
            rc = lib.sir_model_train_bwd(*head, C.byref(g), *tail, st)
        elif fn == "sir_model_train_bwd_part":
            rc = lib.sir_model_train_bwd_part(*head, C.byref(g), *tail, part, st)
        elif fn == "sir_model_train_bwd_cfg":
            rc = lib.sir_model_train_bwd_cfg(*head, cfg, C.byref(g), *tail, part, st)
        else:
            assert fn == "sir_model_train_bwd_x"
            rc = lib.sir_model_train_bwd_x(*head, cfg, C.byref(g), dfeats.data_ptr() if dfeats is not None else None, *tail, part, st)
        torch.cuda.synchronize()
        return rc, buf


def _bits(t):
    return t.view(torch.int32)


def group_variants():
    """The backward against itself at (3, 68) and (2, 257): two halves == whole, a frozen conv2 (NULL pointers) leaves the other
    gradients bit for bit, and one frozen-BatchNorm step against input_grad_ref.reference."""
    from test_input_grad_gpu import _check_step, _model as _ig_model, _step
    sd = _sd()
    for bsz, t in VARIANT_SHAPES:
        f = _Fwd(sd, bsz, t)
        rc, whole = f.call("sir_model_train_bwd_cfg")
        _native.check(rc, "sir_model_train_bwd_cfg")
        assert whole.flat.abs().max().item() > 0 and whole.flat.isfinite().all()
        halves = train_ops.GradBuffer(f.m)
        for part in (_native.BWD_HEAD_GRU, _native.BWD_CNN):
            rc, _ = f.call("sir_model_train_bwd_part", part=part, buf=halves)
            _native.check(rc, "sir_model_train_bwd_part")
        assert torch.equal(_bits(halves.flat), _bits(whole.flat)), (bsz, t)
        for null in (("conv2.weight",), ("conv2.weight", "bn2.weight", "bn2.bias")):
            rc, part = f.call("sir_model_train_bwd_cfg", null=null)
            _native.check(rc, "sir_model_train_bwd_cfg")
            for name, v, v0 in zip(f.names, part.views, whole.views):
                if name in null:
                    assert torch.count_nonzero(v).item() == 0, (bsz, t, name)          # not written
                else:
                    assert torch.equal(_bits(v), _bits(v0)), (bsz, t, null, name)
        print(f"CASE variants B={bsz} T={t}: HEAD_GRU + CNN and two frozen-conv2 calls bit-identical to SIR_BWD_ALL")
        # every BatchNorm on its running statistics, all 29 gradients and dfeats wanted: the affine dz branch in front of the fallbacks
        frozen = (1, 2, 3)
        x, y = _inputs(bsz, t)
        m = _ig_model(sd, frozen_bn=frozen)
        logits, loss, dx = _step(m, x, y)
        _check_step(f"CASE frozen bn{frozen} B={bsz} T={t}", sd, m, x, y, logits, loss, dx, bn_frozen=(True,) * 3)
        ops.check_status()


# ---- inference ---------------------------------------------------------------------------------------------------------------
def _margin(ref):
    top2 = ref.topk(2, dim=1).values
    return top2[:, 0] - top2[:, 1]


def _dense(tag, sd, sharp_sd, x, ref, ref_sharp):
    """test_token_range_gpu.py::test_short_dense_inference_vs_oracle's check, margin rule included"""
    xd = x.contiguous().to(DEV)
    lg, am = _model(sd, False).predict(xd)
    lgs, ams = _model(sharp_sd, False).predict(xd)
    torch.cuda.synchronize()
    err = (lg.cpu().double() - ref).abs().max().item()
    errs = (lgs.cpu().double() - ref_sharp).abs().max().item()
    print(f"CASE dense {tag}: max |logit error| {err:.2e} (init scale; smallest oracle margin {_margin(ref).min().item():.2e}), "
          f"{errs:.2e} (sharp head; smallest oracle margin {_margin(ref_sharp).min().item():.2e})")
    assert _margin(ref).min().item() > 2 * 2e-5 and _margin(ref_sharp).min().item() > 2 * 2e-3      # the argmax is decided
    assert err <= 2e-5
    assert torch.equal(am.cpu(), lg.cpu().argmax(1)) and torch.equal(am.cpu(), ref.argmax(1))
    assert errs < 2e-3
    assert torch.equal(ams.cpu(), ref_sharp.argmax(1))
    ops.check_status()
    return err, errs


def infer_data(sd, sharp_sd):
    """Five clips of 31 frames and their float64 oracle logits at every t of the sweep (a row does not see its batch in eval mode),
    and two clips of 2055 frames: rows 0 and 1 of test_long_sequence_gpu.py's data."""
    from test_token_range_gpu import INFER_TMAX, INFER_TS
    sd64, sharp64 = _f64(sd), _f64(sharp_sd)
    x = cases.varied_features(max(INFER_BATCHES), INFER_TMAX, seed=831).float()
    xl = cases.varied_features(17, 2055, seed=2055).float()[:2].contiguous()
    ref, ref_sharp = {}, {}
    with torch.no_grad():
        for t, xt in [(t, x[:, :, :t]) for t in INFER_TS] + [(2055, xl)]:
            st = {}
            ref[t] = model_ref.forward(sd64, xt.double(), stages=st)
            ref_sharp[t] = st["ctx"] @ sharp64["fc.weight"].t() + sharp64["fc.bias"]
    return {"x": x, "xl": xl, "ref": ref, "ref_sharp": ref_sharp}


def group_infer():
    import test_pad_skip_gpu as ps
    from test_token_range_gpu import INFER_TMAX, INFER_TS, RAGGED_MARGIN, RAGGED_TOL
    sd = _sd()
    sharp_sd = cases.sharp_head(sd, np.load(os.path.join(ROOT, "tests", "golden", "model_golden.npz"))["sharp_fc_bias"])
    d = infer_data(sd, sharp_sd)
    worst = [0.0, 0.0]
    for t in INFER_TS:
        for bsz in INFER_BATCHES:
            e = _dense(f"T={t} B={bsz}", sd, sharp_sd, d["x"][:bsz, :, :t], d["ref"][t][:bsz], d["ref_sharp"][t][:bsz])
            worst = [max(a, b) for a, b in zip(worst, e)]
    e = _dense("T=2055 B=2", sd, sharp_sd, d["xl"], d["ref"][2055], d["ref_sharp"][2055])
    print(f"CASE dense worst T=8..31: {worst[0]:.2e} init scale, {worst[1]:.2e} sharp head; T=2055: {e[0]:.2e}, {e[1]:.2e}")

    # pad skip: +0.0 tails of several extents == the same rows with -0.0 tails (computed in full); position; NaN in a tail
    m = _model(sd, False)
    for t_pad in (24, 200):
        x = ps._feats(PAD_LENGTHS, t_pad)
        ext = ps._extent(x).tolist()
        xf = ps._neg_tail(x)
        assert len(set(ext)) >= 4 and min(ext) < t_pad and not torch.equal(_bits(x), _bits(xf)), ext
        lg, am = ps._infer(m, x)
        lgf, amf = ps._infer(m, xf)
        assert torch.equal(_bits(lg), _bits(lgf)) and torch.equal(am, amf), t_pad
        with torch.no_grad():
            ref = model_ref.forward(_f64(sd), x.cpu().double())
        err = (lg.cpu().double() - ref).abs().max().item()
        assert err <= 2e-4 and not lg.isnan().any()
        perm = torch.randperm(x.shape[0], generator=torch.Generator().manual_seed(3)).to(DEV)
        lgp, _ = ps._infer(m, x[perm].contiguous())
        assert torch.equal(_bits(lg[perm]), _bits(lgp)), t_pad
        short = [b for b, e_ in enumerate(ext) if e_ <= t_pad - 4][:2]
        assert len(short) == 2, ext
        xn = x.clone()
        xn[short[0], 7, t_pad - 2] = float("nan")
        xn[short[1], 0, t_pad - 4] = float("nan")
        lgn, amn = ps._infer(m, xn)
        lgnf, amnf = ps._infer(m, ps._neg_tail(xn))
        assert torch.equal(lgn.isnan(), lgnf.isnan()) and torch.equal(_bits(torch.nan_to_num(lgn)), _bits(torch.nan_to_num(lgnf)))
        assert torch.equal(amn, amnf)
        others = [b for b in range(x.shape[0]) if b not in short]
        assert lgn[short].isnan().all() and torch.equal(_bits(lgn[others]), _bits(lg[others]))     # the NaN is its own rows' alone
        print(f"CASE pad skip t_pad={t_pad}: extents {ext}, +0.0 tails bit-identical to -0.0 tails, to the permuted batch and beside a NaN; "
              f"max |logit error| {err:.2e}")
        ops.check_status()

    # ragged: every clip of the sweep in one batch of 31 frames, NaN behind its length, on a 0xFF-filled workspace
    n = len(INFER_TS)
    x = torch.full((n, 64, INFER_TMAX), float("nan"))
    for i, t in enumerate(INFER_TS):
        x[i, :, :t] = d["x"][0, :, :t]
    ref = torch.stack([d["ref"][t][0] for t in INFER_TS])
    ws = ops.Workspace()
    ws.get(_native.lib().sir_model_workspace_bytes(get_featurizer().handle, n, INFER_TMAX, 0), torch.device(DEV, torch.cuda.current_device())).fill_(0xFF)
    lg, am = ops.model_infer(m, x.to(DEV), ws, want_argmax=True, lengths=torch.tensor(INFER_TS, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    lg, am = lg.cpu(), am.cpu()
    assert not lg.isnan().any()
    err = (lg.double() - ref).abs().max().item()
    clear = _margin(ref) >= RAGGED_MARGIN
    print(f"CASE ragged T=8..31 B={n}: max |logit error| {err:.2e}, {int((~clear).sum())} clips below the argmax margin")
    assert err <= RAGGED_TOL
    assert torch.equal(am[clear], ref.argmax(1)[clear])
    assert int(clear.sum()) >= n // 2
    ops.check_status()


# ---- operand range on the bf16x3 planes ----------------------------------------------------------------------------------------
def group_range():
    """What include/sir_hip.h's operand-range paragraph says of the fallbacks.  The bf16 planes keep fp32's exponent: a transformed
    conv2 weight of 40 is inside their range -- no status bit, exact against float64 (on the default kernels: status bit 3).  A conv2
    block output of 300 raises status bit 12 whatever the plan (the forward's bn_relu_pool_kernel does not know it); with conv3's
    weight gradient on the nine-tap kernel (SIR_CONV_FALLBACK=2) all 29 gradients hold their bound all the same, with it on the
    Winograd f16x3 kernel (=1) conv3.weight's does not, which is what the bit reports."""
    import test_operand_range_gpu as orr
    fallback = int(os.environ["SIR_CONV_FALLBACK"])
    tag = "conv2.weight[0,0,0,0]=40"
    sd = orr._with(orr._sd(), [("conv2.weight", (0, 0, 0, 0), 40.0)])
    orr._inference_vs_oracles("CASE range " + tag, sd)
    ops.check_status()                                   # no bit 3
    s, errs, bounds = orr._training_vs_oracles("CASE range " + tag, sd, f32_bound=True)
    ops.check_status()
    range_ref.assert_backward("CASE range " + tag + " training", *errs, **bounds)

    tag = "bn2.bias[5]=300"
    sd = orr._with(orr._sd(), [("bn2.weight", (5,), 1.0), ("bn2.bias", (5,), 300.0)])
    s, (gerr, nerr, serr), _ = orr._training_vs_oracles("CASE range " + tag, sd, f32_bound=False)
    print(f"CASE range {tag}: max a2 {s.views()['a2'].max().item():.1f}, conv3.weight gradient {gerr['conv3.weight']:.1e} * rms")
    assert s.views()["a2"].max().item() >= 256.0
    try:
        ops.check_status()
        raised = ""
    except _native.SirError as e:
        raised = str(e)
    print(f"CASE range {tag}: check_status: {raised or 'clean'}")
    assert "code -1" in raised and "conv2 block output >= 256" in raised            # status bit 12
    ops.check_status()
    if fallback == 2:
        range_ref.assert_backward("CASE range " + tag + " training", gerr, nerr, serr)
    else:                                                # conv3's weight gradient is the Winograd f16x3 kernel: the reported operand
        rest = {k: v for k, v in gerr.items() if k != "conv3.weight"}
        assert max(rest.values()) < range_ref.GRAD_BOUND, max(rest, key=rest.get)
        assert all(e < range_ref.GRAD_BOUND for e in serr.values()), serr


# ---- the refusal: a row wider than the nine-tap weight-gradient kernel takes ------------------------------------------------------
ENTRY_POINTS = [("sir_model_train_bwd", _native.BWD_ALL, False), ("sir_model_train_bwd_part", _native.BWD_ALL, False),
                ("sir_model_train_bwd_part", _native.BWD_HEAD_GRU, False), ("sir_model_train_bwd_part", _native.BWD_CNN, False),
                ("sir_model_train_bwd_cfg", _native.BWD_ALL, False), ("sir_model_train_bwd_x", _native.BWD_ALL, False),
                ("sir_model_train_bwd_x", _native.BWD_ALL, True)]


def group_refusal():
    assert os.environ.get("SIR_CONV_FALLBACK") == "2"
    sd = _sd()
    lib = _native.lib()
    for bsz, t in REFUSED:
        f = _Fwd(sd, bsz, t)
        zo, yo = f.oracle_values()
        with torch.no_grad():
            ref = model_ref.forward(_f64(sd), f.x.double(), train=True, z_override=_f64(zo), y_override=_f64(yo))
        lerr = (f.logits.cpu().double() - ref).abs().max().item()
        assert lerr < 5e-5, lerr
        buf = train_ops.GradBuffer(f.m)
        dfeats = torch.empty_like(f.xd)
        _bits(buf.flat).fill_(SENTINEL)
        _bits(dfeats).fill_(SENTINEL)
        ws0 = f.ws.clone()
        msgs = []

        def refused():
            for fn, part, with_dx in ENTRY_POINTS:
                rc, _ = f.call(fn, part=part, buf=buf, dfeats=dfeats if with_dx else None)
                msgs.append(lib.sir_last_error().decode(errors="replace"))
                assert rc == _native.SIR_EUNSUPPORTED, (bsz, t, fn, part, rc, msgs[-1])

        refused()                                        # two-stream form
        counts, _ = input_grad_ref.launch_counts(refused)
        assert sum(counts.values()) == 0, {k: v for k, v in counts.items() if v}
        assert bool((_bits(buf.flat) == SENTINEL).all()) and bool((_bits(dfeats) == SENTINEL).all()), (bsz, t)
        assert torch.equal(f.ws, ws0), (bsz, t)          # the workspace too: not a byte
        assert all(f"t_frames={t}" in msg and "weight gradient" in msg for msg in msgs), msgs
        ops.check_status()
        # the torch surface: loss.backward() raises, no .grad appears
        m = _model(sd, True)
        loss = train_ops.fused_cross_entropy(m(f.xd), f.y.to(DEV))
        try:
            loss.backward()
            raised = ""
        except RuntimeError as e:
            raised = str(e)
        assert "code -4" in raised, raised
        assert all(p.grad is None for p in m.parameters())
        ops.check_status()
        print(f"CASE refusal B={bsz} T={t}: forward logits err {lerr:.1e}; {len(ENTRY_POINTS)} backward calls SIR_EUNSUPPORTED, 0 launches, "
              f"gradients, dfeats and workspace untouched")

    # a conv block whose weight gradient is not wanted launches no nine-tap kernel and runs: (1, 520), conv weights frozen, dfeats wanted
    from test_input_grad_gpu import _check_step, _step
    bsz, t = 1, 520
    x, y = _inputs(bsz, t)
    m = _model(sd, True)
    frozen = ("conv1.weight", "conv2.weight", "conv3.weight")
    for n, p in m.named_parameters():
        p.requires_grad_(n not in frozen)
    logits, loss, dx = _step(m, x, y)
    _check_step(f"CASE refusal lifted B={bsz} T={t}, conv weights frozen", sd, m, x, y, logits, loss, dx)
    zo, yo = _device_forward_values(m, sd, x, bsz, t, _views(m, bsz, t))
    _, ref_grads, _, _ = _oracle_f64(sd, x, y, zo, yo)
    worst = 0.0
    for n, p in m.named_parameters():
        if n in frozen:
            assert p.grad is None, n
            continue
        if ref_grads[n].abs().max() <= 1e-7:
            e = float((p.grad.cpu() - ref_grads[n]).abs().max())
        else:
            e = _rel(p.grad, ref_grads[n])[0]
        worst = max(worst, e)
        assert e < range_ref.GRAD_BOUND, (n, e)
    print(f"CASE refusal lifted B={bsz} T={t}: worst of the 26 wanted gradients {worst:.1e} * rms")
    ops.check_status()


# ---- the first shape at which a gate closes by itself ----------------------------------------------------------------------------
def group_natural():
    """Batch 2048 of 256 frames, no switch: conv2's weight gradient alone runs on the nine-tap kernel (tests/test_conv_plan_gates.py
    holds the plan to that).  The gated contraction against float64 formed on the device from the step's own operands."""
    assert "SIR_CONV_FALLBACK" not in os.environ
    bsz, t = NATURAL
    wp1 = t // 2
    sd = _sd()
    x = cases.varied_features(bsz, t, seed=3000 + bsz).to(DEV)
    y = synth.synth_labels(bsz, 31, seed=3001 + bsz).to(DEV)
    m = _model(sd, True)
    t0 = time.perf_counter()
    loss = train_ops.fused_cross_entropy(m(x), y)
    loss.backward()
    torch.cuda.synchronize()
    step_s = time.perf_counter() - t0
    ops.check_status()                                   # SIR_OK: no recurrence timed out
    grads = {n: p.grad for n, p in m.named_parameters()}
    assert len(grads) == 29 and torch.isfinite(loss).item()
    for n, g in grads.items():
        assert g is not None and bool(torch.isfinite(g).all()), n
    offs = input_grad_ref.workspace_offsets(bsz, t)
    ws = m._sir_train["ws"].buf
    scale = range_ref.device_loss_scale(m, bsz, t)
    a1 = ws[offs[0]: offs[0] + 4 * bsz * 32 * wp1 * 32].view(torch.float32).view(bsz, 32, wp1, 32)
    dz2 = ws[offs[28]: offs[28] + 4 * bsz * 32 * wp1 * 64].view(torch.float32).view(bsz * 32 * wp1, 64)
    dz = dz2.double().t().contiguous()                                           # [64][N]
    ap = torch.nn.functional.pad(a1.double(), (0, 0, 1, 1, 1, 1))                # [B][34][wp1 + 2][32]: zero border
    ref = torch.empty(64, 32, 3, 3, dtype=torch.float64, device=DEV)
    for ky in range(3):
        for kx in range(3):
            ref[:, :, ky, kx] = dz @ ap[:, ky:ky + 32, kx:kx + wp1, :].reshape(bsz * 32 * wp1, 32)
    ref /= scale
    got = grads["conv2.weight"].double()
    rms = ref.pow(2).mean().sqrt().item()
    ratio = (got - ref).abs().max().item() / rms
    print(f"CASE natural B={bsz} T={t}: loss {loss.item():.4f}, step {step_s:.2f} s, loss scale 2^{int(np.log2(scale))}, conv2.weight gradient "
          f"max |got - ref| / rms(ref) = {ratio:.2e} (rms {rms:.2e})")
    assert rms > 0 and ratio <= range_ref.GRAD_BOUND
    ops.check_status()


GROUPS = {"train_short": group_train_short, "train_tiles": group_train_tiles, "variants": group_variants, "infer": group_infer,
          "range": group_range, "refusal": group_refusal, "natural": group_natural}


def main(group):
    t0 = time.perf_counter()
    print(f"group {group}, SIR_CONV_FALLBACK={os.environ.get('SIR_CONV_FALLBACK', 'unset')}")
    GROUPS[group]()
    torch.cuda.synchronize()
    print(f"FALLBACK-CASES-OK {group} ({time.perf_counter() - t0:.1f} s)")


if __name__ == "__main__":
    main(sys.argv[1])
