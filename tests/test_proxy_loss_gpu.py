"""GPU: the cosine-proxy loss (``sir_proxy_loss``), the gradient entrance at the embedding (``sir_model_train_bwd_emb``) and their
Python surface (``forward_with_embedding``, ``ProxyHead``, ``metric_loss`` in ``train()``).

The loss kernel is held to tests/proxy_ref.py: the float64 restatement and the bounds derived there (nothing measured on the
kernel enters a bound).  The backward entrance is held to the float64 oracle differentiated at the device's own z / y values, the
yardstick of tests/train_step_ref.py: max |a - ref| <= 2e-3 * rms(ref), absolute where the reference gradient is <= 1e-7.
Every check prints what it measured before it asserts (``-s``).

Measured on MI355X: the loss within 6.8e-7 of float64 (0.42 % of its bound at worst), demb at most 1.0 % of its bound, dproxies
at most 10.5 %; the joint loss through the backward: worst gradient 1.06e-5 (3 x 24), 9.3e-6 (17 x 16), 1.16e-5 (5 x 40 ragged),
dfeats at most 5.7e-6, the proxies' gradient at most 3.2e-6, all times rms; with dlogits all zero at most 1.07e-5; with both
gradients scaled by 2^-24 and 2^16 the same figures to every printed digit."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cases
import input_grad_ref
import proxy_ref
import ragged_grad_ref as rg
from sir_amd import _native, ops, synth, train_ops
from sir_amd.featurizer import get_featurizer
from sir_amd.models.models import CNNAudioGRU
from sir_amd.prototypes import PrototypeBank, ProxyHead

pytestmark = pytest.mark.gpu
DEV = "cuda"
GRAD_BOUND = 2e-3
SCALES, MARGINS = (1.0, 16.0, 64.0), (0.0, 0.2)
SHAPES = [(b, 65) for b in (1, 2, 17, 65, 257)] + [(17, p) for p in (1, 2, 31, 64, 65, 257, 4096)]


# ---- the loss kernel ----------------------------------------------------------------------------------------------------------
def run_loss(emb, proxies, labels, scale, margin, grad_scale=1.0, want_demb=True, want_dprox=True):
    lib, h = _native.lib(), get_featurizer().handle
    e, p = torch.as_tensor(emb).to(DEV).contiguous(), torch.as_tensor(proxies).to(DEV).contiguous()
    y = torch.as_tensor(labels).to(DEV)
    bsz, n = e.shape[0], p.shape[0]
    need = lib.sir_proxy_loss_workspace_bytes(bsz, n)
    assert need > 0
    ws = torch.empty((need,), dtype=torch.uint8, device=DEV)
    loss = torch.empty((), dtype=torch.float32, device=DEV)
    demb = torch.empty_like(e) if want_demb else None
    dprox = torch.empty_like(p) if want_dprox else None
    rc = lib.sir_proxy_loss(h, e.data_ptr(), p.data_ptr(), y.data_ptr(), bsz, n, scale, margin, loss.data_ptr(),
                            demb.data_ptr() if want_demb else None, dprox.data_ptr() if want_dprox else None, grad_scale,
                            ws.data_ptr(), need, _native.current_stream_ptr())
    _native.check(rc, "sir_proxy_loss")
    torch.cuda.synchronize()
    return loss.cpu(), demb.cpu() if want_demb else None, dprox.cpu() if want_dprox else None


def check_against_ref(tag, emb, proxies, labels, scale, margin, grad_scale=1.0):
    ref = proxy_ref.loss_and_grads(emb, proxies, labels, scale, margin, grad_scale)
    loss, demb, dprox = run_loss(emb, proxies, labels, scale, margin, grad_scale)
    lerr, lb = abs(float(loss) - ref["loss"]), proxy_ref.loss_bound(ref, scale)
    eb, pb = proxy_ref.demb_bound(ref, scale), proxy_ref.dproxies_bound(ref, scale)
    ee, pe = np.abs(demb.double().numpy() - ref["demb"]), np.abs(dprox.double().numpy() - ref["dproxies"])
    with np.errstate(invalid="ignore", divide="ignore"):
        er = float(np.nanmax(np.where(eb > 0, ee / eb, np.where(ee > 0, np.inf, 0.0))))
        pr = float(np.nanmax(np.where(pb > 0, pe / pb, np.where(pe > 0, np.inf, 0.0))))
    print(f"{tag} scale={scale} margin={margin}: loss {float(loss):.6f} err {lerr:.2e} (bound {lb:.2e}); worst demb err / bound {er:.3f} "
          f"(max err {ee.max():.2e}), worst dproxies err / bound {pr:.3f} (max err {pe.max():.2e})")
    assert np.isfinite(float(loss)) and lerr <= lb
    assert torch.isfinite(demb).all() and torch.isfinite(dprox).all()
    assert er <= 1.0 and pr <= 1.0
    return loss, demb, dprox, ref


@pytest.mark.parametrize("bsz,n", SHAPES)
def test_loss_and_gradients_vs_float64(bsz, n):
    emb, proxies, labels = proxy_ref.make_case(bsz, n, seed=100 * bsz + n)
    for scale in SCALES:
        for margin in MARGINS:
            loss, demb, dprox, _ = check_against_ref(f"B={bsz} P={n}", emb, proxies, labels, scale, margin)
            if n == 1:                                   # one proxy: softmax = 1 exactly
                assert float(loss) == 0.0
                assert torch.equal(demb, torch.zeros_like(demb)) and torch.equal(dprox, torch.zeros_like(dprox))
    ops.check_status()


def test_null_outputs_change_nothing_else():
    emb, proxies, labels = proxy_ref.make_case(17, 65, seed=7)
    full = run_loss(emb, proxies, labels, 16.0, 0.2)
    for we, wp in ((True, False), (False, True), (False, False)):
        got = run_loss(emb, proxies, labels, 16.0, 0.2, want_demb=we, want_dprox=wp)
        assert torch.equal(got[0], full[0])
        assert (got[1] is None) == (not we) and (got[2] is None) == (not wp)
        assert not we or torch.equal(got[1], full[1])
        assert not wp or torch.equal(got[2], full[2])


def test_ignored_rows_grad_scale_and_norm_extremes():
    emb, proxies, labels = proxy_ref.make_case(17, 65, seed=8, ignore=(0, 5, 16))
    emb[0] = np.nan                                      # an ignored row's embedding is never looked at
    emb[3] *= np.float32(1e-15)
    emb[4] *= np.float32(1e15)
    proxies[2] *= np.float32(1e-15)
    proxies[9] *= np.float32(1e15)
    loss, demb, dprox, ref = check_against_ref("ignored rows, norms 1e-15 / 1e15, grad_scale 0.375", emb, proxies, labels, 16.0, 0.2, 0.375)
    assert ref["n_valid"] == 14
    for b in (0, 5, 16):
        assert torch.equal(demb[b], torch.zeros(512))
    # all rows ignored but one
    labels1 = np.full((17,), -100, np.int64)
    labels1[11] = labels[11]
    _, demb1, _, ref1 = check_against_ref("one labelled row of 17", emb, proxies, labels1, 16.0, 0.0)
    assert ref1["n_valid"] == 1 and int((demb1.abs().sum(dim=1) > 0).sum()) == 1
    # every row ignored: 0 / 0, as sir_ce_loss
    loss0, demb0, dprox0 = run_loss(emb, proxies, np.full((17,), -100, np.int64), 16.0, 0.0)
    assert torch.isnan(loss0) and torch.equal(demb0, torch.zeros_like(demb0)) and torch.equal(dprox0, torch.zeros_like(dprox0))
    ops.check_status()


def test_reproducible_and_row_independent():
    emb, proxies, labels = proxy_ref.make_case(17, 257, seed=9)
    a, b = run_loss(emb, proxies, labels, 16.0, 0.2), run_loss(emb, proxies, labels, 16.0, 0.2)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # row 6 alone, and inside a batch of 17 whose other rows are ignored (n_valid = 1 both times)
    only = np.full((17,), -100, np.int64)
    only[6] = labels[6]
    in_batch = run_loss(emb, proxies, only, 16.0, 0.2)
    alone = run_loss(emb[6:7], proxies, labels[6:7], 16.0, 0.2)
    assert torch.equal(in_batch[0], alone[0]) and torch.equal(in_batch[1][6], alone[1][0]) and torch.equal(in_batch[2], alone[2])


def test_label_out_of_range_raises_status():
    emb, proxies, labels = proxy_ref.make_case(5, 31, seed=10)
    ops.check_status()
    labels[2] = 31
    loss, demb, _ = run_loss(emb, proxies, labels, 16.0, 0.0)
    assert torch.isnan(loss) and torch.isfinite(demb).all()
    with pytest.raises(_native.SirError):
        ops.check_status()
    ops.check_status()                                   # (the word is cleared by the check)


def test_refusals_write_nothing():
    lib, h = _native.lib(), get_featurizer().handle
    bsz, n = 5, 31
    emb, proxies, labels = (torch.as_tensor(v).to(DEV) for v in proxy_ref.make_case(bsz, n, seed=11))
    need = lib.sir_proxy_loss_workspace_bytes(bsz, n)
    assert lib.sir_proxy_loss_workspace_bytes(0, n) == 0 and lib.sir_proxy_loss_workspace_bytes(bsz, 0) == 0
    assert lib.sir_proxy_loss_workspace_bytes(bsz, 4097) == 0 and lib.sir_proxy_loss_workspace_bytes(bsz, 4096) > 0
    canary = 0x5A
    ws = torch.full((need + 64,), canary, dtype=torch.uint8, device=DEV)
    outs = {k: torch.full(s, canary, dtype=torch.uint8, device=DEV) for k, s in
            (("loss", (16,)), ("demb", (bsz * 512 * 4 + 16,)), ("dprox", (n * 512 * 4 + 16,)))}
    st = _native.current_stream_ptr()
    good = dict(h=h, emb=emb.data_ptr(), prox=proxies.data_ptr(), y=labels.data_ptr(), b=bsz, n=n, scale=16.0, margin=0.1,
                loss=outs["loss"].data_ptr(), demb=outs["demb"].data_ptr(), dprox=outs["dprox"].data_ptr(), gs=1.0, ws=ws.data_ptr(),
                wsb=need)
    refusals = {"NULL emb": dict(emb=None), "NULL proxies": dict(prox=None), "NULL labels": dict(y=None), "NULL loss": dict(loss=None),
                "NULL workspace": dict(ws=None), "NULL handle": dict(h=None),
                "misaligned emb": dict(emb=good["emb"] + 4), "misaligned demb": dict(demb=good["demb"] + 4),
                "misaligned dproxies": dict(dprox=good["dprox"] + 8), "misaligned workspace": dict(ws=good["ws"] + 4),
                "misaligned labels": dict(y=good["y"] + 4),
                "batch 0": dict(b=0), "no proxies": dict(n=0), "4097 proxies": dict(n=4097),
                "scale 0": dict(scale=0.0), "scale < 0": dict(scale=-1.0), "scale NaN": dict(scale=float("nan")),
                "margin < 0": dict(margin=-0.1), "workspace too small": dict(wsb=need - 1)}
    for what, change in refusals.items():
        a = dict(good, **change)
        rc = lib.sir_proxy_loss(a["h"], a["emb"], a["prox"], a["y"], a["b"], a["n"], a["scale"], a["margin"], a["loss"], a["demb"],
                                a["dprox"], a["gs"], a["ws"], a["wsb"], st)
        assert rc == _native.SIR_EINVAL, what
    torch.cuda.synchronize()
    for k, v in list(outs.items()) + [("workspace", ws)]:
        assert bool((v == canary).all()), k
    a = good
    rc = lib.sir_proxy_loss(a["h"], a["emb"], a["prox"], a["y"], a["b"], a["n"], a["scale"], a["margin"], a["loss"], a["demb"], a["dprox"],
                            a["gs"], a["ws"], a["wsb"], st)
    assert rc == _native.SIR_OK
    torch.cuda.synchronize()
    assert bool((ws[need:] == canary).all()) and bool((outs["demb"][bsz * 512 * 4:] == canary).all())
    assert bool((outs["dprox"][n * 512 * 4:] == canary).all()) and bool((outs["loss"][4:] == canary).all())
    ops.check_status()


# ---- the backward entrance ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sd():
    return synth.synth_state_dict(31, seed=0)


def _model(sd, frozen):
    if frozen:
        return rg.frozen_model(sd, 0.0)
    m = CNNAudioGRU(31)
    m.load_state_dict(sd)
    m = m.to(DEV).train()
    m.gru.dropout = 0.0
    return m


def _bsc(m, bsz, t, pairs):
    offs = (C.c_size_t * 48)()
    assert _native.lib().sir_model_train_workspace_offsets(get_featurizer().handle, bsz, t, offs, 48) > 39
    return m._sir_train["ws"].buf[offs[39]: offs[39] + 8 * pairs].view(torch.float32).cpu().clone()


OLDER = {(False, False): "sir_model_train_bwd_cfg", (False, True): "sir_model_train_bwd_x", (True, True): "sir_model_train_bwd_ragged"}
NULL_DEMB_CASES = [(3, 24, False, False), (3, 24, False, True), (5, 40, True, True)]


class _HandStep:
    """One case of the two tests below: the Python step once (its ``.grad``s, ``x.grad``, the ``dlogits`` it handed down and slot
    39), then ``by_hand(fn)``: the same forward again and the backward entry point ``fn`` called by hand on the step's own
    workspace, into a second ``GradBuffer`` and a ``dfeats`` pre-filled with NaN."""

    def __init__(self, sd, bsz, t, frozen, want_dx, dropout=0.0):
        self.bsz, self.t, self.want_dx = bsz, t, want_dx
        self.x = cases.varied_features(bsz, t, seed=40 + bsz).float()
        y = synth.synth_labels(bsz, 31, seed=41 + bsz).to(DEV)
        self.frames = torch.tensor([40, 7, 23, 16, 9], dtype=torch.int32, device=DEV) if frozen else None
        self.m = m = _model(sd, frozen)
        m.gru.dropout = dropout
        got = {}
        m.zero_grad(set_to_none=True)
        xd, logits = self.forward()
        logits.register_hook(lambda g: got.__setitem__("dlogits", g.detach().clone()))
        train_ops.fused_cross_entropy(logits, y).backward()
        torch.cuda.synchronize()
        self.dlogits = got["dlogits"]
        self.grads = {n: p.grad.detach().clone() for n, p in m.named_parameters()}
        self.dx = xd.grad.detach().clone() if want_dx else None
        self.bsc = _bsc(m, bsz, t, 1)

    def forward(self):
        train_ops.set_dropout_step(5)                    # (every forward of the case draws the same mask)
        xd = self.x.to(DEV).requires_grad_(self.want_dx)
        return xd, self.m(xd, lengths=self.frames)

    def by_hand(self, fn):
        lib, h, m = _native.lib(), get_featurizer().handle, self.m
        xd, _ = self.forward()
        w, keep = ops.cached_weights(m)
        buf = train_ops.GradBuffer(m)
        buf.flat.fill_(float("nan"))
        dx = torch.full_like(xd, float("nan")) if self.want_dx else None
        ws = m._sir_train["ws"].buf
        seed, p_used = m._sir_last_dropout
        assert p_used == (m.gru.dropout if m.gru.training else 0.0)
        cfg, _ = train_ops.step_config(m)
        head = (h, C.byref(w), ops._as_features(xd.detach()).data_ptr())
        shape = (self.bsz, self.t, p_used, seed, C.byref(cfg), C.byref(buf.struct))
        tail = (ws.data_ptr(), ws.numel(), _native.BWD_ALL, _native.current_stream_ptr())
        dl, dxp = self.dlogits.data_ptr(), dx.data_ptr() if self.want_dx else None
        fp = self.frames.data_ptr() if self.frames is not None else None
        if fn == "sir_model_train_bwd_cfg":
            assert dx is None and fp is None
            rc = lib.sir_model_train_bwd_cfg(*head, dl, *shape, *tail)
        elif fn == "sir_model_train_bwd_x":
            assert fp is None
            rc = lib.sir_model_train_bwd_x(*head, dl, *shape, dxp, *tail)
        elif fn == "sir_model_train_bwd_ragged":
            rc = lib.sir_model_train_bwd_ragged(*head, fp, dl, *shape, dxp, *tail)
        else:
            assert fn == "sir_model_train_bwd_emb"
            rc = lib.sir_model_train_bwd_emb(*head, fp, dl, None, *shape, dxp, *tail)
        _native.check(rc, fn)
        torch.cuda.synchronize()
        return dict(zip((n for n, _ in m.named_parameters()), buf.views)), dx, _bsc(m, self.bsz, self.t, 1)

    def expect_bad_length(self):
        if self.frames is not None:
            with pytest.raises(_native.SirError):        # (the length 7: status bit 6, as the ragged step documents)
                ops.check_status()


@pytest.mark.parametrize("bsz,t,frozen,want_dx", NULL_DEMB_CASES)
def test_null_demb_is_the_existing_backward(sd, bsz, t, frozen, want_dx):
    """``sir_model_train_bwd_emb`` with ``demb == NULL`` against ``_cfg`` (no dfeats), ``_x`` and ``_ragged`` (one length < 8), both
    called by hand (the Python node itself calls ``_emb``): all 29 gradients, dfeats and slot 39 ``torch.equal``."""
    step = _HandStep(sd, bsz, t, frozen, want_dx)
    ref_grads, ref_dx, ref_bsc = step.by_hand(OLDER[(frozen, want_dx)])
    grads, dx, bsc = step.by_hand("sir_model_train_bwd_emb")
    assert torch.equal(bsc, ref_bsc)
    assert len(grads) == 29
    for n, v in grads.items():
        assert torch.equal(v, ref_grads[n]), n
    if want_dx:
        assert torch.equal(dx, ref_dx)
    step.expect_bad_length()


@pytest.mark.parametrize("bsz,t,frozen,want_dx,dropout", [c + (0.0,) for c in NULL_DEMB_CASES] + [(3, 24, False, False, 0.25)])
def test_python_step_is_the_older_entry_point(sd, bsz, t, frozen, want_dx, dropout):
    """What ties the Python node to the C contract: ``m(x, lengths=...)`` then ``fused_cross_entropy(...).backward()`` leaves in every
    ``.grad`` and in ``x.grad`` the bits of the older entry point the case names, called by hand after the same forward with the
    seed and ``p`` of ``m._sir_last_dropout`` (the fourth case: with inter-layer dropout 0.25)."""
    step = _HandStep(sd, bsz, t, frozen, want_dx, dropout)
    ref_grads, ref_dx, ref_bsc = step.by_hand(OLDER[(frozen, want_dx)])
    assert torch.equal(step.bsc, ref_bsc)
    assert len(step.grads) == 29
    for n, v in step.grads.items():
        assert torch.equal(v, ref_grads[n]), n
    if want_dx:
        assert torch.equal(step.dx, ref_dx)
    step.expect_bad_length()


def _joint_step(m, head, x, y, frames, ce, factor):
    m.zero_grad(set_to_none=True)
    head.zero_grad(set_to_none=True)
    xd = x.to(DEV).requires_grad_(True)
    train_ops.set_dropout_step(5)
    logits, emb = m.forward_with_embedding(xd, lengths=frames)
    loss = head(emb, y)
    if ce:
        loss = loss + train_ops.fused_cross_entropy(logits, y)
    (loss * factor).backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), xd.grad.detach().cpu(), emb.detach().cpu()


def _joint_check(tag, sd, m, head, x, y, frames, ce, factor=1.0):
    bsz, t = x.shape[0], x.shape[-1]
    flist = [int(f) for f in frames.tolist()] if frames is not None else None
    loss, dx, emb = _joint_step(m, head, x, y, frames, ce, factor)
    xz = rg.zero_tails(x, flist) if flist is not None else x
    zo, yo = input_grad_ref.device_forward_values(m, sd, xz, bsz, t)
    ref_loss, ref_grads, ref_dx, ref_dp = proxy_ref.joint_reference(sd, x, y.cpu(), head.proxies, head.scale, head.margin, zo, yo,
                                                                    frames=flist, ce_weight=1.0 if ce else 0.0)
    errs = {}
    unscale = 1.0 / factor                               # (a power of two: exact)
    for n, p in m.named_parameters():
        g = p.grad.detach().cpu().double() * unscale
        # the yardstick of tests/train_step_ref.py: absolute where the reference gradient is <= 1e-7, else relative to its rms
        errs[n] = float((g - ref_grads[n]).abs().max()) if ref_grads[n].abs().max() <= 1e-7 else rg.ratio(g, ref_grads[n])
    errs["dx"] = rg.ratio(dx.double().view(ref_dx.shape) * unscale, ref_dx)
    errs["proxies"] = rg.ratio(head.proxies.grad.detach().cpu().double() * unscale, ref_dp)
    worst = max(errs, key=errs.get)
    print(f"{tag}: loss err {abs(float(loss) - float(ref_loss)):.2e}; worst {worst} {errs[worst]:.2e}; dx {errs['dx']:.2e}; "
          f"proxies {errs['proxies']:.2e}; fc.weight {errs['fc.weight']:.2e}; conv1.weight {errs['conv1.weight']:.2e}")
    assert len(errs) == 31
    assert abs(float(loss) - float(ref_loss)) <= 2e-5 * max(1.0, abs(float(ref_loss)))
    for k, v in errs.items():
        assert v <= GRAD_BOUND, (k, v)
    return errs


@pytest.mark.parametrize("bsz,t,frozen", [(3, 24, False), (17, 16, False), (5, 40, True)])
@pytest.mark.parametrize("ce", [True, False])
def test_joint_loss_vs_float64_oracle(sd, bsz, t, frozen, ce):
    """CE + ProxyHead (``ce``) and ProxyHead alone (dlogits all zero) through the whole backward: all 29 gradients, dfeats and the
    proxies' gradient."""
    x = cases.varied_features(bsz, t, seed=60 + bsz).float()
    y = synth.synth_labels(bsz, 31, seed=61 + bsz).to(DEV)
    frames = torch.tensor([40, 8, 23, 16, 9], dtype=torch.int32, device=DEV) if frozen else None
    m = _model(sd, frozen)
    head = ProxyHead(31, scale=16.0, margin=0.1, seed=3).to(DEV)
    _joint_check(f"B={bsz} T={t} frozen={frozen} ce={ce}", sd, m, head, x, y, frames, ce)
    ops.check_status()


@pytest.mark.parametrize("k", [-24, 16])
@pytest.mark.parametrize("ce", [True, False])
def test_joint_loss_scaled_by_powers_of_two(sd, k, ce):
    """(dlogits, demb) scaled jointly by 2^k, with the classifier's loss and without it, against the same bound."""
    x = cases.varied_features(3, 24, seed=63).float()
    y = synth.synth_labels(3, 31, seed=64).to(DEV)
    m = _model(sd, False)
    head = ProxyHead(31, scale=16.0, margin=0.1, seed=3).to(DEV)
    _joint_check(f"B=3 T=24 x 2^{k} ce={ce}", sd, m, head, x, y, None, ce, factor=2.0 ** k)
    ops.check_status()


def test_per_row_mode_rows_are_independent(sd):
    """All 29 gradients NULL, frozen statistics, dfeats wanted: row b's dfeats carries the same bits alone and in a batch of 3, with
    the gradient entering at the embedding (and slot 39 holds a pair per row)."""
    lib, h = _native.lib(), get_featurizer().handle
    t = 24
    x = cases.varied_features(3, t, seed=70).float().to(DEV)
    g = torch.Generator().manual_seed(71)
    demb = (torch.randn(3, 512, generator=g) * torch.tensor([[1e-6], [1.0], [300.0]])).to(DEV)
    dlogits = (torch.randn(3, 31, generator=g) * 1e-3).to(DEV)
    m = rg.frozen_model(sd, 0.0)
    cfg, _ = train_ops.step_config(m)
    none = _native.ModelGrads()

    def run(rows):
        xr = x[rows].contiguous()
        n = xr.shape[0]
        leaf = xr.detach().requires_grad_(True)
        with torch.enable_grad():
            train_ops.forward_craft(m, leaf)             # the training-path forward with no side effect: fills the workspace
        w, keep = ops.cached_weights(m)
        ws = m._sir_train["ws"].buf
        dx = torch.full_like(xr, float("nan"))
        de, dl = demb[rows].contiguous(), dlogits[rows].contiguous()
        rc = lib.sir_model_train_bwd_emb(h, C.byref(w), xr.data_ptr(), None, dl.data_ptr(), de.data_ptr(), n, t, 0.0, 0, C.byref(cfg),
                                         C.byref(none), dx.data_ptr(), ws.data_ptr(), ws.numel(), _native.BWD_ALL,
                                         _native.current_stream_ptr())
        _native.check(rc, "sir_model_train_bwd_emb")
        torch.cuda.synchronize()
        return dx.cpu(), _bsc(m, n, t, 1 + n)

    full, bsc = run([0, 1, 2])
    print("per-row scales:", bsc.view(-1, 2)[:, 0].tolist())
    assert torch.isfinite(full).all() and len(set(bsc.view(-1, 2)[1:, 0].tolist())) == 3
    for b in range(3):
        alone, bsc1 = run([b])
        assert torch.equal(alone[0], full[b]), b
        assert torch.equal(bsc1.view(-1, 2)[1], bsc.view(-1, 2)[1 + b])
    ops.check_status()


# ---- surface ------------------------------------------------------------------------------------------------------------------
def test_forward_with_embedding_in_eval(sd):
    m = _model(sd, False).eval()
    x = cases.varied_features(5, 40, seed=80).float().to(DEV)
    logits, emb = m.forward_with_embedding(x)
    assert torch.equal(logits, m(x)) and torch.equal(emb, m.embed(x))
    assert not logits.requires_grad and not emb.requires_grad
    m.train()
    with torch.no_grad():
        l2, e2 = m.forward_with_embedding(x)
    assert torch.equal(l2, logits) and torch.equal(e2, emb)


def test_training_embedding_is_the_workspace_context(sd):
    """The second output is a copy (the next step must not change it) and CE alone through the two-output node is
    ``forward_train``'s step bit for bit."""
    m = _model(sd, False)
    x = cases.varied_features(3, 24, seed=81).float().to(DEV)
    y = synth.synth_labels(3, 31, seed=82).to(DEV)
    m.zero_grad(set_to_none=True)
    train_ops.fused_cross_entropy(m(x), y).backward()
    ref = {n: p.grad.detach().clone() for n, p in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    logits, emb = m.forward_with_embedding(x)
    kept = emb.detach().clone()
    train_ops.fused_cross_entropy(logits, y).backward()
    for n, p in m.named_parameters():
        assert torch.equal(p.grad, ref[n]), n
    m(cases.varied_features(3, 24, seed=83).float().to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(emb.detach(), kept) and emb.shape == (3, 512)


@pytest.fixture
def new_process():
    """The dropout step counter as a new process has it (1), put back afterwards."""
    before = train_ops.dropout_step()
    train_ops.set_dropout_step(1)
    yield
    train_ops.set_dropout_step(before)


def test_train_with_metric_loss_and_resume(tmp_path, new_process):
    """``train()`` with ``metric_loss`` on a synthetic split (two steps an epoch): a clean status word, ``proxy_head.pt`` and
    ``bank_out`` written, the bank ranks every proxy's own row first, and a run resumed after two epochs ends on the bits of the
    run that went straight through three."""
    import json
    import types

    import pandas as pd

    from sir_amd import run_state
    from sir_amd.scripts import precompute_features as pf
    from sir_amd.scripts import train as tr
    from test_pipeline_gpu import LABELS, _make_corpus

    rows = _make_corpus(str(tmp_path / "wav"))
    csvs = {}
    for split, sl in (("train", slice(0, 16)), ("valid", slice(16, 20))):
        p = tmp_path / f"{split}_data.csv"
        pd.DataFrame(rows[sl]).to_csv(p, index=False)
        csvs[split] = str(p)
        pf.precompute_dataset_features(str(p), str(tmp_path / "cache"))
    lm = tmp_path / "label_map.json"
    lm.write_text(json.dumps({l: i for i, l in enumerate(sorted(LABELS))}))
    args = types.SimpleNamespace(train_csv=csvs["train"], val_csv=csvs["valid"], label_map=str(lm))
    cfg = {"batch_size": 8, "num_workers": 0, "num_labels": 31, "lr": 1e-3, "weight_decay": 1e-2, "early_stop_patience": 5,
           "augment_prob": 0.7, "cache_dir": str(tmp_path / "cache"), "use_feature_cache": True, "seed": 2,
           "metric_loss": {"weight": 1.0, "ce_weight": 0.5, "scale": 16, "margin": 0.1, "bank_out": "proxies.npz"},
           "checkpoint_every_epoch": True}

    def run(save_dir, **kw):
        torch.manual_seed(1234)
        train_ops.set_dropout_step(1)
        return tr.train(args, dict(cfg, save_path=str(tmp_path / save_dir), **kw))

    run("resumed", epochs=2)
    first = torch.load(tmp_path / "resumed" / run_state.PROXY_HEAD, weights_only=True)
    init = ProxyHead(31, scale=16.0, margin=0.1, seed=2)
    assert first["proxies"].shape == (31, 512) and not torch.equal(first["proxies"], init.proxies.detach())    # (they were trained)
    run("resumed", epochs=3, resume=True)
    run("straight", epochs=3)
    ops.check_status()
    a = torch.load(tmp_path / "resumed" / run_state.LATEST, weights_only=False)
    b = torch.load(tmp_path / "straight" / run_state.LATEST, weights_only=False)
    assert a["epoch"] == b["epoch"] == 2
    for k, v in a["model_state_dict"].items():
        assert torch.equal(v, b["model_state_dict"][k]), k
    for g in ("_sir_group_0", "_sir_group_1"):
        sa, sb = a["optimizer_state_dict"]["state"][g], b["optimizer_state_dict"]["state"][g]
        assert sa["step"] == sb["step"] == 6
        assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]), g
    ha, hb = (torch.load(tmp_path / d / run_state.PROXY_HEAD, weights_only=True) for d in ("resumed", "straight"))
    assert torch.equal(ha["proxies"], hb["proxies"]) and ha["names"] == hb["names"] and ha["scale"] == 16.0 and ha["margin"] == 0.1
    bank = PrototypeBank.load(tmp_path / "straight" / "proxies.npz")
    assert bank.names == hb["names"] and len(bank.names) == 31
    scores = bank.score(hb["proxies"].to(DEV), k=1)
    assert torch.equal(scores.classes[:, 0].cpu(), torch.arange(31, dtype=torch.int32))
    assert float(scores.sims[:, 0].min()) > 1.0 - 1e-5
    # the model from the metric run still loads as the reference's bare state dict where one was saved
    best = tmp_path / "straight" / "best_model.pt"
    if best.exists():
        assert list(torch.load(best)) == list(synth.synth_state_dict(31).keys())
