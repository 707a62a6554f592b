"""The feature kernels at every frame count, against float64 (inputs and references: tests/frame_count_ref.py).

``feat_utt_kernel`` / ``feat_utt_bwd_kernel`` branch on the clip's frame count T = 1 + L // 512 alone: which waves of a round of 16
transform and which prefetch, whether the dB tile stays in registers (T <= 160) or is parked in the output row, how many live
lanes the last round has, where the trim and the padding fall, how many carries the overlap-add passes on, and where the reflected
tail lands.  The forward is run at every T from 2 to 176 and both ends of each hop, the backward at every T from 2 to 49 and around
64, 96, 128, 160 and 176; the general front ends (tiles of 64 frames) at every frame count up to 130.

Bounds.
* Forward: the project's ``|a - ref| <= 1e-4 * max(1, |ref|)`` on the dB values and on the normalised output, every element,
  taken against FLOAT64 (``oracle.features_ref.extract_features_f64``; ``frontend_cfg_ref.features_f64`` on the general front
  ends).  The float32 oracle itself uses up to 0.6e-4 of that against float64 on these inputs (tests/test_frame_count_host.py),
  which is why the kernel is not compared with it; every test prints the kernel's worst value and the float32 oracle's beside it.
* Backward: ``clip_error = max |a - ref64| / rms(ref64)`` of the kernel is at most 4 x that of the float32 autograd gradient of
  the same clip (the rule of tests/test_features_grad_gpu.py).  A lost overlap-add contribution is an error of order 1 under
  this measure, five orders above the bound.
  Two places where that rule says nothing, and what stands there instead:
  - A shift of +-(L - 1) leaves one sample of the clip, the gradient has ONE non-zero element, and clip_error is that element's
    relative error times sqrt(L).  The clip's own float32 yardstick is then a single rounding draw: at L = 513, shift -512, float32
    autograd landed 1.8e-8 from float64 (a sixth of an ulp) and the kernel 1.8e-7 (ratio 9.9); at L = 8191, shift -8190, 7.3e-8
    against 4.2e-7 (ratio 5.8).  Neither is a lost contribution (that is an error of the whole element, sqrt(L) >= 22 under the
    measure), so for the clips of this kind the yardstick is the largest float32 error among them (6.7e-2, an ill-conditioned
    element at L = 81919, shift +81918), factor 4 kept: the element must be right to 0.27 / sqrt(L), 1.2 % at L = 513.  Every
    other augmented clip is held to its own yardstick (worst ratio 1.39).
  - L = 512 (T - 1): the last padded sample folds back onto 512 (T - 2) - 1 through one thread after the loop.  Its Hann weight
    is 9.4e-6; under a full ``dout`` it is 7e-7 (at most 1.7e-5) of the clip's rms, below the rounding of the sample it lands on,
    and the parity test passes without it.  ``test_backward_folds_the_last_padded_sample`` feeds the last frame alone, takes the
    fold from the float64 reference differentiated at the padded clip, and regresses the kernel's error at that sample on it:
    +0.0007 measured, -1.000 with the fix-up deleted, bound 0.5.
* Everything said to be equal is compared bit for bit; everything said to be zero is an exact zero.

Measured on MI355X (worst over each sweep; the float32 oracle's own figure on the same clips in brackets):
  forward float32   dB 5.91e-5 at T = 75, L = 37888, filter 54, frame 74 (5.96e-5); normalised 1.16e-5 at T = 166, L = 84480 (1.16e-5)
  forward int16     dB 6.02e-5 at T = 75, L = 37888, filter 54, frame 74 (5.92e-5); normalised 1.15e-5 at T = 82, L = 41542 (1.16e-5)
  augmented forward normalised 1.72e-5 at T = 160, L = 81408, shift -81407
  general 512/160/400    dB 8.2e-6 at 44 frames (9.4e-6);  normalised 3.0e-6 (3.5e-6)
  general 256/64/256     dB 1.08e-5 at 8 frames (1.07e-5); normalised 9.7e-6 (9.7e-6)
  general 1024/256/1024  dB 1.02e-5 at 91 frames (1.31e-5); normalised 1.1e-6 (1.2e-6)
  backward float32  err(GPU) / err(float32 autograd): worst 1.46 at T = 20, L = 10239, median 1.00
  backward int16    worst 1.18 at T = 129, L = 66047, median 0.99
The forward's worst clip is the float32 oracle's worst clip too: the kernel is as far from float64 as ``torch.stft`` in float32
is, 0.6 of the tolerance.  No frame count, hop offset, row alignment or t_pad stands out, and no defect was found in
csrc/features_fwd.hip / features_bwd.hip (then one file, csrc/features.hip).

Three arithmetic-only mutations of that file (now features_bwd.hip, features_fwd.hip and feat_common.h), each built once on a scratch copy and run against this module: without the
``L == (T - 1) * SIR_HOP`` fix-up ``test_backward_folds_the_last_padded_sample`` fails (coefficient -1.000) and nothing else;
``q * NW + mf <= T`` in the forward's statistics fails ``test_forward_every_frame_count`` (normalised 1.1e-1 at T = 2) and
``test_augmentation_at_the_edges``; ``2 * L - 1 - i`` in ``fetch`` fails the forward (10 dB in the last frame), backward (ratio
6.6e5), fold, augmentation and general-front-end tests.
"""
import numpy as np
import pytest
import torch

import features_grad_ref as gref
import frame_count_ref as fc
from sir_amd import _native, featurizer

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 1e-4
FACTOR = 4.0
SENT = 12345.5
T_PAD = fc.T_PAD
ALONE_T = (2, 16, 17, 160, 161, 176)


def _rows(values, width):
    """CPU [N, L] -> device view [N, L] of a zeroed [N, width] buffer: the row stride is ``width`` samples."""
    buf = torch.zeros(values.shape[0], width, dtype=values.dtype, device=DEV)
    view = buf[:, : values.shape[1]]
    view.copy_(values)
    return view


def _even(n):
    return n + (n & 1)


def _lens(lens):
    return torch.tensor(list(lens), dtype=torch.int32, device=DEV)


def _fwd(view, lens, t_pad=T_PAD, fz=None, **aug):
    """One forward launch into NaN-filled ``out`` and ``db_out``; CPU results."""
    fz = fz or featurizer.get_featurizer()
    out = torch.full((view.shape[0], 64, t_pad), float("nan"), device=DEV)
    db = torch.full((view.shape[0], 64, t_pad), float("nan"), device=DEV)
    fz(view, _lens(lens), t_pad=t_pad, out=out, db_out=db, **aug)
    torch.cuda.synchronize()
    return out.cpu(), db.cpu()


def _bwd(view, lens, dout, t_pad=T_PAD, extra=16, **aug):
    """Forward (keeping db) + ``sir_features_bwd`` into a [N, L + extra] buffer pre-filled with a sentinel; CPU (out, dwave)."""
    fz = featurizer.get_featurizer()
    ld = _lens(lens)
    db = torch.empty(view.shape[0], 64, t_pad, device=DEV)
    out = fz(view, ld, t_pad=t_pad, db_out=db, **aug)
    buf = torch.full((view.shape[0], view.shape[1] + extra), SENT, device=DEV)
    fz.features_bwd(view, ld, db, dout.to(DEV), t_pad=t_pad, out=buf, **aug)
    torch.cuda.synchronize()
    return out.cpu(), buf.cpu()


def _src(ref, kind):
    return ref["pcm"] if kind == "i16" else ref["wave"]


# ---- forward ---------------------------------------------------------------------------------------------------------------
FWD_CASES = fc.fwd_cases()
FWD_LENS = [n for _, n in FWD_CASES]
FWD_LMAX = max(FWD_LENS)


class _Once(dict):
    """{kind: result}, each computed when it is first asked for and kept for the module."""

    def __init__(self, make):
        super().__init__()
        self.make = make

    def __missing__(self, kind):
        self[kind] = self.make(kind)
        return self[kind]


@pytest.fixture(scope="module")
def fwd():
    """The forward sweep from even-width buffers: {kind: (out, db)} float32 [N, 64, 176] on the CPU."""
    return _Once(lambda kind: _fwd(_rows(_src(fc.fwd_reference(kind), kind), _even(FWD_LMAX)), FWD_LENS))


def _worst(err, frames):
    i, f, t = np.unravel_index(np.argmax(err), err.shape)
    return f"{err[i, f, t]:.3e} (T = {frames[i]}, clip {i}, filter {f}, frame {t})", i


def _check_against_f64(tag, out, db, ref, lens, t_pad):
    out, db = out.numpy(), db.numpy()
    frames = ref["frames"]
    valid = np.arange(t_pad)[None, None, :] < frames[:, None, None]
    valid = np.broadcast_to(valid, out.shape)
    assert np.isfinite(out).all() and np.isfinite(db).all(), tag
    assert (out[~valid] == 0).all() and (db[~valid] == 0).all(), tag             # exact zeros behind every clip
    e_db = fc.measure(db, ref["db64"][:, :, :t_pad]) * valid
    e_out = fc.measure(out, ref["norm64"][:, :, :t_pad]) * valid
    w_db, i_db = _worst(e_db, frames)
    w_out, i_out = _worst(e_out, frames)
    print(f"{tag}: kernel against float64, worst dB {w_db} L = {lens[i_db]}; worst normalised {w_out} L = {lens[i_out]}; "
          f"float32 oracle against float64: dB {ref['o32_db'].max():.3e}, normalised {ref['o32_norm'].max():.3e}")
    assert e_db.max() <= TOL, (tag, w_db, lens[i_db])
    assert e_out.max() <= TOL, (tag, w_out, lens[i_out])


@pytest.mark.parametrize("kind", ["f32", "i16"])
def test_forward_every_frame_count(fwd, kind):
    out, db = fwd[kind]
    _check_against_f64(f"forward {kind}", out, db, fc.fwd_reference(kind), FWD_LENS, T_PAD)


def test_alignment_odd_row_width_and_int16_against_float32(fwd):
    """An odd row width puts every second row off the sample-pair boundary (``load_frame``'s element loads, for int16 a row on a
    2-byte boundary): the same bits.  int16 input and float32 input of the same values q / 32768 feed the transform the same
    floats: the same bits."""
    for kind in ("f32", "i16"):
        src = _src(fc.fwd_reference(kind), kind)
        odd = _rows(src, _even(FWD_LMAX) + 1)
        assert odd.stride(0) % 2 == 1
        out, db = _fwd(odd, FWD_LENS)
        assert torch.equal(out, fwd[kind][0]) and torch.equal(db, fwd[kind][1]), kind
    deq = fc.fwd_reference("i16")["wave"]
    for width in (_even(FWD_LMAX), _even(FWD_LMAX) + 1):
        out, db = _fwd(_rows(deq, width), FWD_LENS)
        assert torch.equal(out, fwd["i16"][0]) and torch.equal(db, fwd["i16"][1]), width


@pytest.mark.parametrize("t_pad", [1, 15, 16, 17, 200])
def test_trim_and_pad(fwd, t_pad):
    """The clips of up to 160 frames at other t_pad: the first t_pad columns of the 176-column result (the statistics run over all
    frames before the trim), zeros behind -- also past column 160, where the padding loop takes over from the register tile."""
    keep = [i for i, (t, _) in enumerate(FWD_CASES) if t <= 160]
    lens = [FWD_LENS[i] for i in keep]
    lmax = max(lens)
    assert 1 + lmax // fc.HOP == 160
    for kind in ("f32", "i16"):
        src = _src(fc.fwd_reference(kind), kind)[keep][:, :lmax]
        out, db = _fwd(_rows(src, _even(lmax)), lens, t_pad=t_pad)
        n = min(t_pad, T_PAD)
        assert torch.equal(out[:, :, :n], fwd[kind][0][keep][:, :, :n]), (kind, t_pad)
        assert torch.equal(db[:, :, :n], fwd[kind][1][keep][:, :, :n]), (kind, t_pad)
        assert (out[:, :, n:] == 0).all() and (db[:, :, n:] == 0).all(), (kind, t_pad)


def test_a_parked_clip_needs_a_slot_per_frame():
    """T = 161 at t_pad = 160: refused, nothing written."""
    cases = [(160, fc.last_len(160)), (161, fc.first_len(161))]
    wave = torch.zeros(2, cases[1][1])
    for i, (t, n) in enumerate(cases):
        wave[i, :n] = fc.clip(t, n)
    out = torch.full((2, 64, 160), SENT, device=DEV)
    db = torch.full((2, 64, 160), SENT, device=DEV)
    with pytest.raises(_native.SirError):
        featurizer.get_featurizer()(wave.to(DEV), _lens(n for _, n in cases), t_pad=160, out=out, db_out=db)
    torch.cuda.synchronize()
    assert (out == SENT).all() and (db == SENT).all()


# ---- backward --------------------------------------------------------------------------------------------------------------
BWD_CASES = fc.bwd_cases()
BWD_LENS = [n for _, n in BWD_CASES]
BWD_LMAX = max(BWD_LENS)


@pytest.fixture(scope="module")
def bwd():
    """The backward sweep from even-width buffers: {kind: dwave float32 [N, Lmax + 16]} on the CPU."""
    def run(kind):
        ref = fc.bwd_reference(kind)
        return _bwd(_rows(_src(ref, kind), _even(BWD_LMAX)), BWD_LENS, ref["dout"])[1]
    return _Once(run)


def _check_gradients(tag, got, g64, e32, lens, labels, yard=None):
    """Prints every clip's figures, then asserts err(GPU) <= 4 x err(float32 autograd) clip by clip (``yard``: a yardstick
    other than the clip's own float32 error; the printed ratios are against the clip's own in every case)."""
    bad, ratios = [], []
    yard = e32 if yard is None else yard
    for i, n in enumerate(lens):
        assert torch.isfinite(got[i, :n]).all(), (tag, labels[i])
        egpu = gref.clip_error(got[i, :n], g64[i])
        ratios.append(egpu / e32[i])
        print(f"{tag} {labels[i]}: err(GPU) = {egpu:.3e}, err(float32 autograd) = {e32[i]:.3e}, ratio {ratios[-1]:.2f}")
        if not egpu <= FACTOR * yard[i]:
            bad.append((labels[i], egpu, e32[i], yard[i]))
    w = int(np.argmax(ratios))
    print(f"{tag}: worst ratio {ratios[w]:.2f} at {labels[w]}, median {np.median(ratios):.2f}")
    assert not bad, (tag, bad)


@pytest.mark.parametrize("kind", ["f32", "i16"])
def test_backward_frame_counts(bwd, kind):
    got, ref = bwd[kind], fc.bwd_reference(kind)
    assert (got[:, BWD_LMAX:] == SENT).all()                        # columns at or beyond max_len are not touched
    for i, n in enumerate(BWD_LENS):
        assert (got[i, n:BWD_LMAX] == 0).all(), (kind, n)           # exact zeros behind the clip
    _check_gradients(f"backward {kind}", got, ref["g64"], ref["e32"], BWD_LENS, [f"T={t} L={n}" for t, n in BWD_CASES])


@pytest.mark.parametrize("kind", ["f32", "i16"])
def test_backward_folds_the_last_padded_sample(kind):
    """L = 512 (T - 1): the last padded sample reflects onto 512 (T - 2) - 1, a block written before frame T - 1 is there when
    that frame opens a round; one thread adds it after the loop.  Its Hann weight is 9.4e-6, so the parity test above cannot
    see it go missing; here ``dout`` feeds the last frame only and the float64 reference says what the fold is
    (``frame_count_ref.fold_reference``).  The kernel's error at that sample, regressed on the fold over all clips, is 0 when the
    fold is there and -1 when it is lost: the bound is the midpoint (float32 autograd measures 7e-4)."""
    ref, cases = fc.fold_reference(kind), fc.fold_cases()
    lens = [n for _, n in cases]
    got = _bwd(_rows(_src(ref, kind), _even(max(lens))), lens, ref["dout"])[1]
    err, fold = np.zeros(len(cases)), np.zeros(len(cases))
    for i, (t, n) in enumerate(cases):
        g, k = ref["g64"][i], fc.fold_sample(t)
        rms = g.pow(2).mean().sqrt().item()
        err[i], fold[i] = (got[i, k].item() - g[k].item()) / rms, ref["fold"][i] / rms
    coef = (err * fold).sum() / (fold * fold).sum()
    print(f"fold {kind}: |fold| / rms median {np.median(np.abs(fold)):.2e}, max {np.abs(fold).max():.2e}; kernel error at the sample / rms "
          f"median {np.median(np.abs(err)):.2e}, max {np.abs(err).max():.2e}; regression coefficient {coef:+.4f}; "
          f"clips with |error| < |fold| / 2: {int((np.abs(err) < np.abs(fold) / 2).sum())} of {len(cases)}")
    assert abs(coef) <= 0.5, coef


def test_backward_odd_row_width(bwd):
    ref = fc.bwd_reference("f32")
    odd = _rows(ref["wave"], _even(BWD_LMAX) + 1)
    assert torch.equal(_bwd(odd, BWD_LENS, ref["dout"])[1], bwd["f32"])
    ref = fc.bwd_reference("i16")
    odd = _rows(ref["pcm"], _even(BWD_LMAX) + 1)
    assert torch.equal(_bwd(odd, BWD_LENS, ref["dout"])[1], bwd["i16"])


def test_row_independence(fwd, bwd):
    """A row's bits depend on nothing but the row: alone (another max_len, another grid) it gives what it gave in the batch."""
    wave_f, wave_b = fc.fwd_reference("f32")["wave"], fc.bwd_reference("f32")
    for i, (t, n) in enumerate(FWD_CASES):
        if t in ALONE_T and n != fc.mid_len(t):
            out, db = _fwd(wave_f[i: i + 1, :n].to(DEV), [n])
            assert torch.equal(out[0], fwd["f32"][0][i]) and torch.equal(db[0], fwd["f32"][1][i]), (t, n)
    for i, (t, n) in enumerate(BWD_CASES):
        if t in ALONE_T:
            _, g = _bwd(wave_b["wave"][i: i + 1, :n].to(DEV), [n], wave_b["dout"][i: i + 1], extra=0)
            assert torch.equal(g[0], bwd["f32"][i, :n]), (t, n)


def test_augmentation_at_the_edges():
    """Shifts that leave one sample of the clip (either way), one short of a hop, one past it and an odd one; noise; a time mask
    from the last frame across the clip's end; a freq mask across mel 64 -- forward and backward against float64."""
    cases, ref = fc.aug_cases(), fc.aug_reference()
    lens = [n for _, n, _ in cases]
    lmax = max(lens)
    nb = len(cases)
    aug = dict(shift=torch.tensor([s for _, _, s in cases], dtype=torch.int32), noise_sigma=torch.full((nb,), fc.AUG_SIGMA),
               noise_seed=fc.AUG_SEED, time_mask=torch.tensor([fc.aug_time_mask(t) for t, _, _ in cases], dtype=torch.int32),
               freq_mask=torch.tensor([fc.AUG_FREQ_MASK] * nb, dtype=torch.int32))
    out, got = _bwd(_rows(ref["wave"], _even(lmax)), lens, ref["dout"], **aug)
    out = out.numpy()
    assert np.isfinite(out).all()
    frames = np.array([t for t, _, _ in cases])
    live = ~ref["constant"]
    assert (out[ref["constant"]] == 0).all() and (got[torch.from_numpy(ref["constant"]), :lmax] == 0).all()   # sigma == 0: constants
    masked = np.zeros(out.shape, dtype=bool)
    for i, t in enumerate(frames):
        masked[i, :, t - 1:] = True                                 # the last frame (time mask) and everything behind the clip
    masked[:, fc.AUG_FREQ_MASK[0]:, :] = True
    assert (out[masked] == 0).all()
    e = fc.measure(out, ref["out64"])[live]
    w, i = _worst(e, frames[live])
    print(f"augmented forward: kernel against float64, worst normalised {w}, case {[c for c, l in zip(cases, live) if l][i]}")
    assert e.max() <= TOL, w
    assert (got[:, lmax:] == SENT).all()
    dead = torch.from_numpy(ref["dead"])
    assert (got[dead, :lmax] == 0).all()                            # the whole clip shifted out: no sample feeds anything
    for i, (t, n, s) in enumerate(cases):
        assert (got[i, n:lmax] == 0).all(), (t, n, s)
        # samples shifted out of the clip feed nothing
        assert (got[i, max(n - s, 0): n] == 0).all() if s > 0 else (got[i, : min(-s, n)] == 0).all(), (t, n, s)
    # A shift of +-(L - 1) leaves ONE sample of the clip: the gradient has one non-zero element, and clip_error is that element's
    # relative error times sqrt(L).  The clip's own float32 yardstick is then a single rounding draw, which can land anywhere down
    # to zero (module docstring), so those clips are held to the largest float32 error among them instead; the factor 4 stays.
    for single in (False, True):
        idx = [i for i in range(nb) if live[i] and not ref["dead"][i] and (abs(cases[i][2]) == cases[i][1] - 1) == single]
        e32 = ref["e32"][idx]
        _check_gradients("augmented backward" + (", one sample left" if single else ""), got[idx], [ref["g64"][i] for i in idx],
                         e32, [lens[i] for i in idx], [f"T={cases[i][0]} L={cases[i][1]} shift={cases[i][2]}" for i in idx],
                         yard=np.full(len(idx), e32.max()) if single else None)


# ---- general front ends ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", fc.GEN_CFGS, ids=lambda c: "n%d_h%d_w%d" % c)
def test_general_front_ends_every_frame_count(cfg):
    ref = fc.gen_reference(cfg)
    fz = featurizer.get_featurizer(16000, 64, *cfg)
    lens = [int(w.numel()) for w in ref["waves"]]
    lmax = max(lens)
    wave = torch.zeros(len(lens), lmax)
    for i, w in enumerate(ref["waves"]):
        wave[i, : w.numel()] = w
    out, db = _fwd(_rows(wave, _even(lmax)), lens, t_pad=fc.GEN_T_PAD, fz=fz)
    _check_against_f64(f"general {cfg}", out, db, ref, lens, fc.GEN_T_PAD)
    for j in fc.gen_empty_filters(cfg):                             # a filter without a bin: exactly -100 dB wherever a frame exists
        for i, t in enumerate(ref["frames"]):
            assert (db[i, j, :t] == -100.0).all()
    out48, db48 = _fwd(_rows(wave, _even(lmax)), lens, t_pad=48, fz=fz)          # statistics over all frames, then the trim
    assert torch.equal(out48, out[:, :, :48]) and torch.equal(db48, db[:, :, :48])
    for i, t in enumerate(ref["frames"]):
        assert (out48[i, :, t:] == 0).all() and (db48[i, :, t:] == 0).all()
    out_odd, db_odd = _fwd(_rows(wave, _even(lmax) + 1), lens, t_pad=fc.GEN_T_PAD, fz=fz)
    assert torch.equal(out_odd, out) and torch.equal(db_odd, db)
