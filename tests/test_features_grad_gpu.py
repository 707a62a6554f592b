"""The feature extractor differentiated down to the waveform (``sir_features_bwd``, ``feat_utt_bwd_kernel``) and the surface on
top of it: ``HipFeaturizer.differentiable``, ``explain.wave_gradient``, ``explain.fgsm_wave``.

Reference: ``tests/features_grad_ref.py`` -- the feature path in torch float64, differentiated by autograd.  The error of a clip is
``max |a - ref64| / rms(ref64)`` over its samples.  Bound: not a constant -- the float32 autograd gradient of
``oracle.features_ref.extract_features_f32`` (``torch.stft``) is measured against the same float64 reference in the same test, and
the kernel may be at most 4 x as far off (a different FFT factorisation and summation order at equal precision).  Every parity
test prints both errors.
"""
import ctypes as C

import pytest
import torch

import features_grad_ref as ref
import host_rng
from sir_amd import _native, explain, ops, synth, train_ops
from sir_amd.featurizer import get_featurizer
from sir_amd.models.models import CNNAudioGRU

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 12345.5
FACTOR = 4.0

LENS1 = [513, 1024, 1535, 7680, 8192, 9000, 512, 20000]      # T = 2; a multiple of the hop; odd; one round; a carry; odd; zero row; clamped
MAX1, TPAD1 = 9000, 24


def _clips(lens, max_len, seed):
    w = torch.zeros(len(lens), max_len)
    for i, n in enumerate(lens):
        n = min(n, max_len)
        w[i, :n] = ref.tones_and_noise(n, seed=seed + i)
    return w


def _dout(bsz, t_pad, seed):
    return torch.randn(bsz, 64, t_pad, generator=torch.Generator().manual_seed(seed))


def _gpu_grad(wave, lens, dout, t_pad, extra=0, **aug):
    """features forward (keeping db) + sir_features_bwd into a [B, L + extra] buffer pre-filled with a sentinel; CPU result."""
    fz = get_featurizer()
    wd = wave.to(DEV)
    ld = torch.tensor(lens, dtype=torch.int32, device=DEV)
    db = torch.empty(wd.shape[0], 64, t_pad, device=DEV)
    fz(wd, ld, t_pad=t_pad, db_out=db, **aug)
    buf = torch.full((wd.shape[0], wd.shape[1] + extra), SENT, device=DEV)
    fz.features_bwd(wd, ld, db, dout.to(DEV), t_pad=t_pad, out=buf, **aug)
    torch.cuda.synchronize()
    return buf.cpu()


def _check(tag, got, x, dout, **kw):
    """got: the kernel's gradient of clip x [L] (float32 values the kernel saw); asserts err(GPU) <= 4 x err(float32 autograd)."""
    g64 = ref.grad_f64(x, dout, **kw)
    e32 = ref.clip_error(ref.grad_f32(x, dout, **kw), g64)
    egpu = ref.clip_error(got, g64)
    print(f"{tag}: err(GPU) = {egpu:.3e}, err(float32 autograd) = {e32:.3e}, ratio {egpu / e32:.2f} (rms {g64.pow(2).mean().sqrt().item():.2e})")
    assert torch.isfinite(got).all()
    assert egpu <= FACTOR * e32, (tag, egpu, e32)


@pytest.fixture(scope="module")
def case1():
    wave = _clips(LENS1, MAX1, seed=100)
    dout = _dout(len(LENS1), TPAD1, seed=1)
    pcm = (wave * 32767.0).round().to(torch.int16)
    return {"wave": wave, "dout": dout, "pcm": pcm,
            "f32": _gpu_grad(wave, LENS1, dout, TPAD1, extra=16),
            "i16": _gpu_grad(pcm, LENS1, dout, TPAD1, extra=16)}


@pytest.mark.parametrize("kind", ["f32", "i16"])
def test_parity_mixed_lengths(case1, kind):
    got, dout = case1[kind], case1["dout"]
    x_all = case1["wave"] if kind == "f32" else case1["pcm"].float() / 32768.0
    assert (got[:, MAX1:] == SENT).all()                      # columns at or beyond max_len are not touched
    for b, n in enumerate(LENS1):
        n = min(n, MAX1)
        assert (got[b, n:MAX1] == 0).all(), (kind, n)         # exact zeros behind the clip
        if n <= 512:
            assert (got[b, :MAX1] == 0).all()                 # the forward's zero row is a constant
            continue
        _check(f"{kind} L={LENS1[b]}", got[b, :n], x_all[b, :n], dout[b])


def test_long_clip():
    """T = 163 frames: more than the forward keeps in registers (its parked path), 11 rounds here."""
    n, t_pad = 83000, 168
    wave = _clips([n], n, seed=200)
    dout = _dout(1, t_pad, seed=2)
    got = _gpu_grad(wave, [n], dout, t_pad)
    _check(f"long L={n}", got[0], wave[0], dout[0])


def test_augmentation():
    lens, shifts, sigma, seed, t_pad = [8192, 8192, 5000, 5000], [300, -700, 300, -700], 5e-3, 77, 20
    tmask, fmask = (3, 4), (10, 6)
    wave = _clips(lens, 8192, seed=300)
    dout = _dout(4, t_pad, seed=3)
    dout[:, :, 3:7] = 1e6                                     # masked positions: must not leak
    dout[:, 10:16, :] = -1e6
    got = _gpu_grad(wave, lens, dout, t_pad,
                    shift=torch.tensor(shifts, dtype=torch.int32), noise_sigma=torch.full((4,), sigma), noise_seed=seed,
                    time_mask=torch.tensor([tmask] * 4, dtype=torch.int32), freq_mask=torch.tensor([fmask] * 4, dtype=torch.int32))
    for b, (n, s) in enumerate(zip(lens, shifts)):
        noise = torch.from_numpy(host_rng.gauss_noise(seed, b, n)).double() * sigma
        assert (got[b, n:] == 0).all()
        _check(f"aug L={n} shift={s}", got[b, :n], wave[b, :n], dout[b], shift=s, noise=noise, time_mask=tmask, freq_mask=fmask)
        # samples shifted out of the clip feed nothing
        assert (got[b, n - s: n] == 0).all() if s > 0 else (got[b, : -s] == 0).all()


def test_clamp_and_degenerate_statistics():
    n, t_pad = 10240, 24
    wave = _clips([n, 2048], n, seed=400)
    wave[0, 3072:7168] = 0.0                                  # frames 7 .. 13 are exact zeros: -100 dB, no gradient
    wave[1] = 0.0                                             # a constant dB tile: sigma == 0
    dout = _dout(2, t_pad, seed=4)
    got = _gpu_grad(wave, [n, 2048], dout, t_pad)
    _check("silent middle", got[0], wave[0], dout[0])
    assert (got[0, 3584:6656] == 0).all()                     # samples only silent frames see
    assert (got[1] == 0).all()                                # exactly zero everywhere, no NaN


def test_determinism_and_independence(case1):
    again = _gpu_grad(case1["wave"], LENS1, case1["dout"], TPAD1, extra=16)
    assert torch.equal(again, case1["f32"])
    for b in range(len(LENS1)):
        alone = _gpu_grad(case1["wave"][b: b + 1], LENS1[b: b + 1], case1["dout"][b: b + 1], TPAD1)
        assert torch.equal(alone[0], case1["f32"][b, :MAX1]), b


def test_refusals_launch_nothing(case1):
    lib, fz = _native.lib(), get_featurizer()
    wd = case1["wave"].to(DEV)
    ld = torch.tensor(LENS1, dtype=torch.int32, device=DEV)
    bsz = wd.shape[0]
    db = torch.zeros(bsz, 64, TPAD1, device=DEV)
    dout = case1["dout"].to(DEV)
    buf = torch.full((bsz, MAX1), SENT, device=DEV)

    def call(db_ptr=db.data_ptr(), t_pad=TPAD1, dstride=MAX1, dtype=_native.WAVE_F32):
        return lib.sir_features_bwd(fz.handle, wd.data_ptr(), dtype, wd.stride(0), ld.data_ptr(), bsz, MAX1, db_ptr, dout.data_ptr(),
                                    t_pad, None, buf.data_ptr(), dstride, _native.current_stream_ptr())

    assert call(t_pad=17) == _native.SIR_EUNSUPPORTED         # 1 + 9000 // 512 = 18 frames
    assert call(db_ptr=None) == _native.SIR_EINVAL
    assert call(dstride=MAX1 - 1) == _native.SIR_EINVAL
    assert call(dtype=7) == _native.SIR_EINVAL
    torch.cuda.synchronize()
    assert (buf == SENT).all()
    assert call() == _native.SIR_OK                           # (the same arguments, un-broken, do launch)
    torch.cuda.synchronize()
    assert not (buf == SENT).any()


# ---- surface -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sd():
    return synth.synth_state_dict(31, seed=0)


def _model(sd):
    m = CNNAudioGRU(31)
    m.load_state_dict(sd)
    m = m.to(DEV).train()
    m.gru.dropout = 0.0
    return m


SLENS, SMAX, STPAD = [8000, 6000, 7001, 8000], 8000, 16


def test_differentiable_matches_the_entry_points_by_hand(sd):
    fz, lib = get_featurizer(), _native.lib()
    wave = _clips(SLENS, SMAX, seed=500).to(DEV)
    ld = torch.tensor(SLENS, dtype=torch.int32, device=DEV)
    y = synth.synth_labels(4, 31, seed=501).to(DEV)

    def step(m, feats):
        m.zero_grad(set_to_none=True)
        train_ops.fused_cross_entropy(m(feats), y).backward()
        torch.cuda.synchronize()

    # through autograd
    ma = _model(sd)
    leaf = wave.clone().requires_grad_(True)
    feats = fz.differentiable(leaf, ld, t_pad=STPAD)
    assert feats.grad_fn is not None
    step(ma, feats)
    assert leaf.grad is not None and leaf.grad.shape == wave.shape
    # by hand: sir_features_fwd with db_out, the training step with x.grad (sir_model_train_bwd_x), sir_features_bwd
    mb = _model(sd)
    db = torch.empty(4, 64, STPAD, device=DEV)
    x = fz(wave, ld, t_pad=STPAD, db_out=db)
    assert x.grad_fn is None and torch.equal(x, feats.detach())        # __call__: the same bits, not a graph node
    x.requires_grad_(True)
    step(mb, x)
    dwave = torch.empty_like(wave)
    _native.check(lib.sir_features_bwd(fz.handle, wave.data_ptr(), _native.WAVE_F32, wave.stride(0), ld.data_ptr(), 4, SMAX,
                                       db.data_ptr(), x.grad.data_ptr(), STPAD, None, dwave.data_ptr(), dwave.stride(0),
                                       _native.current_stream_ptr()), "sir_features_bwd")
    torch.cuda.synchronize()
    assert dwave.abs().max() > 0 and torch.equal(leaf.grad, dwave)
    # the parameters' gradients do not notice
    mc = _model(sd)
    step(mc, fz(wave, ld, t_pad=STPAD))
    for (n, p), (_, q), (_, r) in zip(ma.named_parameters(), mb.named_parameters(), mc.named_parameters()):
        assert torch.equal(p.grad, r.grad) and torch.equal(q.grad, r.grad), n
    # once differentiable
    leaf2 = wave.clone().requires_grad_(True)
    out = fz.differentiable(leaf2, ld, t_pad=STPAD)
    (g,) = torch.autograd.grad(out.sum(), leaf2, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()
    ops.check_status()


def test_wave_gradient_and_fgsm_wave(sd):
    fz = get_featurizer()
    wave = _clips(SLENS, SMAX, seed=510).to(DEV)
    ld = torch.tensor(SLENS, dtype=torch.int32, device=DEV)
    target = torch.tensor([3, 30, 0, 17], device=DEV)
    m = _model(sd)
    step_y = synth.synth_labels(4, 31, seed=511).to(DEV)
    train_ops.fused_cross_entropy(m(fz(wave, ld, t_pad=STPAD)), step_y).backward()      # gradients in place, train() mode
    grads = {n: p.grad for n, p in m.named_parameters()}
    kept = {n: g.clone() for n, g in grads.items()}
    stats = {k: v.clone() for k, v in m.state_dict().items()}
    flags = {n: mod.training for n, mod in m.named_modules()}
    counter = train_ops.dropout_step()

    logits, dwave = explain.wave_gradient(m, wave, ld, target, t_pad=STPAD)
    db = torch.empty(4, 64, STPAD, device=DEV)
    feats = fz(wave, ld, t_pad=STPAD, db_out=db)
    logits_x, dx = explain.input_gradient(m, feats, target)
    by_hand = fz.features_bwd(wave, ld, db, dx, t_pad=STPAD)
    torch.cuda.synchronize()
    assert dwave.shape == wave.shape and not dwave.requires_grad
    assert torch.equal(logits, logits_x) and torch.equal(dwave, by_hand) and dwave.abs().max() > 0
    for b, n in enumerate(SLENS):
        assert (dwave[b, n:] == 0).all()

    eps = 1e-3
    assert torch.equal(explain.fgsm_wave(m, wave, step_y, 0.0, lengths=ld, t_pad=STPAD), wave)
    adv = explain.fgsm_wave(m, wave, step_y, eps, lengths=ld, t_pad=STPAD)
    inside = torch.arange(SMAX, device=DEV)[None, :] < ld[:, None]
    assert torch.equal(adv[~inside], wave[~inside])
    assert adv.min() >= -1.0 and adv.max() <= 1.0
    moved = (adv != wave) & inside
    assert moved.float().sum() > 0.9 * inside.float().sum()
    assert ((adv - wave).abs()[moved] <= eps * (1 + 1e-3) + 2.0 ** -24).all()
    tight = explain.fgsm_wave(m, wave, step_y, eps, lengths=ld, t_pad=STPAD, clamp=(-0.05, 0.05))
    assert tight[inside].min() >= -0.05 and tight[inside].max() <= 0.05
    loose = explain.fgsm_wave(m, wave * 20.0, step_y, eps, lengths=ld, t_pad=STPAD, clamp=None)
    assert loose.abs().max() > 1.0

    # the module is as it was: mode flags, running statistics, p.grad, the dropout counter
    assert {n: mod.training for n, mod in m.named_modules()} == flags
    for n, p in m.named_parameters():
        assert p.grad is grads[n] and torch.equal(p.grad, kept[n]), n
    for k, v in stats.items():
        assert torch.equal(m.state_dict()[k], v), k
    assert train_ops.dropout_step() == counter
    ops.check_status()
