"""GPU: utterance embeddings (sir_model_embed) and the prototype head (sir_proto_reset / _accumulate / _finalize / _score,
sir_amd.prototypes, the callers' prototypes= keyword) against the float64 restatement in proto_ref.py.

Bounds (proto_ref.py derives them): SIM_BOUND = 600 * 2^-24 absolute on every similarity and class score,
prob_bound(p) = (exp(2 * scale * SIM_BOUND) - 1) * p + 4 * 2^-24 on every probability.  Rankings are checked with no case left
out (proto_ref.check_ranking).  Bit-exact where the header promises bits: cut invariance of the bank, batch-position invariance
of the scores, the embedding against the workspace's context rows, logits against sir_model_infer."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import cases
import proto_ref
from oracle import model_ref
from proto_ref import SIM_BOUND, prob_bound
from sir_amd import _native, ops, synth
from sir_amd.featurizer import get_featurizer
from sir_amd.models.models import CNNAudioGRU
from sir_amd.prototypes import PrototypeBank, fit_scale

pytestmark = pytest.mark.gpu
DEV = "cuda"
DIM = 512
SENTINEL = 0x5A


def _lib():
    return _native.lib()


def _h():
    return get_featurizer().handle


def _st():
    return _native.current_stream_ptr()


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _rows(n, seed):
    return np.random.Generator(np.random.PCG64(seed)).standard_normal((n, DIM)).astype(np.float32)


def _unit32(x):
    return proto_ref.unit_rows(x)[0].astype(np.float32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if a is not None else None


# ---- raw calls ---------------------------------------------------------------------------------------------------------------
def _new_state(P):
    n = _lib().sir_proto_state_bytes(P)
    assert n == 64 + 8 * P + 8 * DIM * P
    state = torch.full((n,), SENTINEL, dtype=torch.uint8, device=DEV)
    assert _lib().sir_proto_reset(_h(), state.data_ptr(), n, P, None, _st()) == 0
    return state


def _parts(state, P):
    """(skipped, count int64 [P], sum float64 [P, 512]) on the host"""
    skipped = int(state[8:16].view(torch.int64).item())
    count = state[64: 64 + 8 * P].view(torch.int64).cpu().numpy()
    total = state[64 + 8 * P: 64 + 8 * P + 8 * DIM * P].view(torch.float64).view(P, DIM).cpu().numpy()
    return skipped, count, total


def _accumulate(state, P, emb, labels):
    emb, labels = _dev(emb), _dev(np.asarray(labels, np.int64))
    rc = _lib().sir_proto_accumulate(_h(), state.data_ptr(), state.numel(), P, emb.data_ptr(), labels.data_ptr(), emb.shape[0], _st())
    assert rc == 0, _lib().sir_last_error()


def _finalize(state, P):
    protos = torch.empty((P, DIM), dtype=torch.float32, device=DEV)
    live = torch.empty((P,), dtype=torch.uint8, device=DEV)
    assert _lib().sir_proto_finalize(_h(), state.data_ptr(), state.numel(), P, protos.data_ptr(), live.data_ptr(), _st()) == 0
    return protos, live


def _score(emb, protos, live=None, pclass=None, n_classes=None, scale=None, k=3):
    """sir_proto_score on device tensors -> dict of host arrays (sims, cls, sim, prob, nearest)"""
    bsz, P = emb.shape[0], protos.shape[0]
    n_classes = P if n_classes is None else n_classes
    sims = torch.empty((bsz, P), dtype=torch.float32, device=DEV)
    cls = torch.empty((bsz, k), dtype=torch.int32, device=DEV)
    sim = torch.empty((bsz, k), dtype=torch.float32, device=DEV)
    prob = torch.empty((bsz, k), dtype=torch.float32, device=DEV)
    nearest = torch.empty((bsz,), dtype=torch.int32, device=DEV)
    sc = torch.full((1,), float(scale), dtype=torch.float32, device=DEV) if scale is not None else None
    rc = _lib().sir_proto_score(_h(), emb.data_ptr(), bsz, protos.data_ptr(), _ptr(live), _ptr(pclass), P, n_classes, _ptr(sc), k,
                                sims.data_ptr(), cls.data_ptr(), sim.data_ptr(), prob.data_ptr(), nearest.data_ptr(), _st())
    assert rc == 0, _lib().sir_last_error()
    return {"sims": sims.cpu().numpy(), "cls": cls.cpu().numpy(), "sim": sim.cpu().numpy(), "prob": prob.cpu().numpy(),
            "nearest": nearest.cpu().numpy()}


# ---- 1. sir_model_embed --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sd():
    return synth.synth_state_dict(31, seed=0)


def _model(sd, num_classes=31):
    m = CNNAudioGRU(num_classes)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def _maxerr(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return ((a - b).abs() / b.abs().clamp(min=1.0)).max().item()


def _lengths(bsz, t, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    f = rng.integers(8, t + 1, size=bsz).tolist()
    f[0] = t
    f[-1] = 8 if bsz > 1 else t
    return f


def _oracle_ctx(sd, x, frames):
    with torch.no_grad():
        if frames is None:
            st = {}
            model_ref.forward(sd, x, stages=st)
            return st["ctx"]
        rows = []
        for b, f in enumerate(frames):
            st = {}
            model_ref.forward(sd, x[b:b + 1, :, :f], stages=st)
            rows.append(st["ctx"][0])
        return torch.stack(rows)


@pytest.mark.parametrize("ragged", [False, True], ids=["padded", "ragged"])
@pytest.mark.parametrize("bsz,t", [(1, 8), (3, 94), (17, 200)])
def test_embedding_is_the_context_row_and_logits_keep_their_bits(sd, bsz, t, ragged):
    x = cases.varied_features(bsz, t, seed=40 + bsz)
    frames = _lengths(bsz, t, bsz) if ragged else None
    lens = torch.tensor(frames, dtype=torch.int32, device=DEV) if ragged else None
    m, xd = _model(sd), x.to(DEV)
    dbg = {}
    emb, logits, amax = ops.model_embed(m, xd, m._ws, lengths=lens, want_logits=True, debug=dbg)
    assert emb.shape == (bsz, DIM) and torch.equal(emb, dbg["ctx"])              # the bits of workspace slot 6
    err = _maxerr(emb, _oracle_ctx(sd, x, frames))
    print(f"embedding vs oracle ctx: {err:.2e}")
    assert err <= 1e-4
    want_logits, want_amax = ops.model_infer(m, xd, m._ws, want_argmax=True, lengths=lens)
    assert torch.equal(logits, want_logits) and torch.equal(amax, want_amax)
    assert torch.equal(m.embed(xd, lengths=lens), emb)                              # without the classifier: the same rows
    assert torch.equal(ops.model_infer(m, xd, m._ws, lengths=lens), want_logits)    # and the workspace still serves sir_model_infer
    ops.check_status()


@pytest.mark.parametrize("ragged", [False, True], ids=["padded", "ragged"])
def test_a_nan_feature_makes_exactly_its_row_nan(sd, ragged):
    x = cases.varied_features(3, 94, seed=43)
    lens = torch.tensor([94, 50, 8], dtype=torch.int32, device=DEV) if ragged else None
    m = _model(sd)
    clean = m.embed(x.to(DEV), lengths=lens)
    x[1, 20, 30] = float("nan")
    emb, logits, _ = ops.model_embed(m, x.to(DEV), m._ws, lengths=lens, want_logits=True)
    assert emb[1].isnan().all() and logits[1].isnan().all()
    assert torch.equal(emb[[0, 2]], clean[[0, 2]]) and not logits[[0, 2]].isnan().any()
    ops.check_status()


def test_a_ragged_length_of_7_makes_its_row_nan_and_raises_at_check_status(sd):
    x = cases.varied_features(3, 94, seed=43).to(DEV)
    m = _model(sd)
    clean = m.embed(x, lengths=torch.tensor([94, 50, 8], dtype=torch.int32, device=DEV))
    emb = m.embed(x, lengths=torch.tensor([94, 7, 8], dtype=torch.int32, device=DEV))
    assert emb[1].isnan().all() and torch.equal(emb[[0, 2]], clean[[0, 2]])
    with pytest.raises(_native.SirError):
        ops.check_status()
    ops.check_status()


# ---- 2. cut invariance -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def enrol_rows():
    """300 random rows over 7 classes; five of them are skipped: a -1 label, a label equal to P, a NaN row, an infinity row and
    a zero row"""
    x = _rows(300, 20)
    labels = np.random.Generator(np.random.PCG64(21)).integers(0, 7, size=300).astype(np.int64)
    labels[5], labels[77] = -1, 7
    x[33, 100] = np.nan
    x[150, 0] = np.inf
    x[299] = 0.0
    bad = np.zeros(300, bool)
    bad[[5, 77, 33, 150, 299]] = True
    return x, labels, bad


def _enrol(x, labels, cuts, P=7):
    state = _new_state(P)
    at = 0
    for n in cuts:
        _accumulate(state, P, x[at:at + n], labels[at:at + n])
        at += n
    assert at == x.shape[0]
    return state


def test_state_is_bit_identical_however_the_rows_are_cut(enrol_rows):
    x, labels, bad = enrol_rows
    whole = _enrol(x, labels, [300])
    for cuts in ([1, 299], [7, 64, 229], [1] * 40 + [260]):
        assert torch.equal(_enrol(x, labels, cuts), whole), cuts
    skipped, count, total = _parts(whole, 7)
    assert skipped == 5
    # the same enrolment without the five rows: the same sums and counts
    s2, c2, t2 = _parts(_enrol(x[~bad], labels[~bad], [295]), 7)
    assert s2 == 0 and np.array_equal(c2, count) and np.array_equal(t2, total)
    ref_t, ref_c = np.zeros((7, DIM)), np.zeros((7,), np.int64)
    assert proto_ref.accumulate(ref_t, ref_c, x, labels) == 5
    assert np.array_equal(count, ref_c)
    rel = np.abs(total - ref_t).max() / np.abs(ref_t).max()
    print(f"sum vs float64 reference: {rel:.2e} relative")
    assert np.abs(total - ref_t).max() <= 1e-12 * np.abs(ref_t).max()


# ---- 3. finalize -------------------------------------------------------------------------------------------------------------
def _ulp_err(a, b):
    """largest |a - b| in units of the fp32 ulp of b (b float32)"""
    return (np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(b), np.float32(2.0 ** -126)))).max()


def test_finalize_empty_class_masked_reset_and_scaled_rows(enrol_rows):
    x, labels, bad = enrol_rows
    P = 9                                                            # classes 7 and 8 stay empty (the label 7 becomes a 9: still outside)
    state = _enrol(x, np.where(labels == 7, 9, labels), [300], P)
    protos, live = _finalize(state, P)
    _, count, total = _parts(state, P)
    ref_p, ref_l = proto_ref.finalize(total, count)
    assert live.cpu().numpy().tolist() == ref_l.tolist() == [1] * 7 + [0, 0]
    assert not protos[7:].any()
    err = _ulp_err(protos.cpu().numpy()[:7], ref_p[:7])
    print(f"prototypes vs reference: {err:.2f} ulp")
    assert err <= 1.0
    # a masked reset clears exactly the masked classes
    before = state.clone()
    mask = torch.tensor([0, 1, 0, 0, 1, 0, 0, 0, 0], dtype=torch.uint8, device=DEV)
    assert _lib().sir_proto_reset(_h(), state.data_ptr(), state.numel(), P, mask.data_ptr(), _st()) == 0
    s1, c1, t1 = _parts(state, P)
    s0, c0, t0 = _parts(before, P)
    keep = mask.cpu().numpy() == 0
    assert s1 == s0 == 5 and np.array_equal(c1[keep], c0[keep]) and np.array_equal(t1[keep], t0[keep])
    assert not c1[~keep].any() and not t1[~keep].any()
    protos2, live2 = _finalize(state, P)
    assert live2.cpu().numpy().tolist() == [1, 0, 1, 1, 0, 1, 1, 0, 0] and torch.equal(protos2[keep], protos[keep])
    # rows at 1e-30 and at 1e30 enrol like any other: the norm is a double
    good, gl = x[~bad], labels[~bad]
    base = _finalize(_enrol(good, gl, [295]), 7)[0].cpu().numpy()
    for factor in (1e-30, 1e30):
        scaled = (good * np.float32(factor)).astype(np.float32)
        assert np.isfinite(scaled).all() and (scaled != 0).any(axis=1).all()
        st = _enrol(scaled, gl, [295])
        assert _parts(st, 7)[0] == 0
        ref_t, ref_c = np.zeros((7, DIM)), np.zeros((7,), np.int64)
        proto_ref.accumulate(ref_t, ref_c, scaled, gl)
        got = _finalize(st, 7)[0].cpu().numpy()
        assert _ulp_err(got, proto_ref.finalize(ref_t, ref_c)[0]) <= 1.0
        # the fp32 scaling rounds the inputs (2^-24 relative each), so against the unscaled bank the prototype moves by a few ulp
        assert np.abs(got - base).max() <= 16 * 2.0 ** -24


# ---- 4. score parity -------------------------------------------------------------------------------------------------------
def _class_maps(P, rng):
    """(name, proto_class or None, n_classes): class = row; many prototypes per class; one class owning all; classes with none"""
    maps = [("identity", None, P)]
    if P >= 2:
        nc = max(1, P // 4)
        maps.append(("many_per_class", rng.integers(0, nc, size=P).astype(np.int32), nc))
        maps.append(("classes_with_none", (2 * rng.integers(0, max(1, P // 8), size=P)).astype(np.int32), max(2, P // 2)))
    maps.append(("one_class_owns_all", np.zeros((P,), np.int32), 1))
    return maps


def _check_scores(got, ref, scale, k, tag):
    s, prob = ref["s"], ref["prob"]
    n_present = int(ref["present"].sum())
    assert np.abs(got["sims"] - ref["sims"]).max() <= SIM_BOUND, tag
    for b in range(s.shape[0]):
        msg = proto_ref.check_ranking(s[b], got["cls"][b], k)
        assert msg is None, (tag, b, msg)
        n = min(k, n_present)
        c = got["cls"][b, :n]
        assert (np.abs(got["sim"][b, :n] - s[b, c]) <= SIM_BOUND).all(), (tag, b)
        assert (np.abs(got["prob"][b, :n] - prob[b, c]) <= prob_bound(prob[b, c], scale)).all(), (tag, b, got["prob"][b], prob[b, c])
        assert not got["sim"][b, n:].any() and not got["prob"][b, n:].any(), (tag, b)      # -1 / 0 / 0 behind the present classes
        near = int(got["nearest"][b])
        if n == 0:
            assert near == -1, (tag, b)
            continue
        assert 0 <= near < ref["cls"].shape[0] and ref["cls"][near] == c[0], (tag, b, near)  # a live prototype of the rank-0 class
        assert abs(ref["sims"][b, near] - s[b, c[0]]) <= 2 * SIM_BOUND, (tag, b, near)


SHAPES = [(b, 65) for b in (1, 2, 15, 16, 17, 63, 64, 65, 257)] + [(17, p) for p in (1, 2, 63, 64, 255, 256, 257, 4096)]


@pytest.mark.parametrize("bsz,P", SHAPES)
def test_scores_match_the_float64_reference(bsz, P):
    rng = np.random.Generator(np.random.PCG64(1000 * bsz + P))
    emb = (_rows(bsz, 3 * bsz + P) * rng.uniform(0.1, 30.0, size=(bsz, 1)).astype(np.float32)).astype(np.float32)
    protos = _unit32(_rows(P, 7 * P + bsz))
    holes = (rng.uniform(size=P) > 0.3).astype(np.uint8)
    holes[rng.integers(0, P)] = 1                                    # (at least one live prototype)
    emb_d, protos_d = _dev(emb), _dev(protos)
    worst, ref_sims = 0.0, proto_ref.similarities(emb, protos)
    for (name, pclass, nc), live in itertools.product(_class_maps(P, rng), (None, holes)):
        pclass_d, live_d = _dev(pclass), _dev(live)
        for scale in (None, 1.0, 16.0, 64.0):
            ref = proto_ref.score(emb, protos, live, pclass, nc, scale=1.0 if scale is None else scale, sims=ref_sims)
            for k in (1, 3, 8):
                got = _score(emb_d, protos_d, live_d, pclass_d, nc, scale, k)
                worst = max(worst, np.abs(got["sims"] - ref["sims"]).max())
                _check_scores(got, ref, 1.0 if scale is None else scale, k, (name, live is not None, k, scale))
    print(f"B={bsz} P={P}: max |sim error| {worst:.2e} (bound {SIM_BOUND:.2e})")


def test_no_live_prototype_at_all():
    emb, protos = _dev(_rows(3, 1)), _dev(_unit32(_rows(5, 2)))
    got = _score(emb, protos, live=torch.zeros(5, dtype=torch.uint8, device=DEV), k=3)
    assert (got["cls"] == -1).all() and not got["sim"].any() and not got["prob"].any() and (got["nearest"] == -1).all()
    assert np.isfinite(got["sims"]).all()


# ---- 5. exact properties -----------------------------------------------------------------------------------------------------
def _same_bits(a, b, rows_a, rows_b):
    return all(np.array_equal(a[key][rows_a].view(np.int32), b[key][rows_b].view(np.int32)) for key in a)


def test_a_rows_outputs_do_not_depend_on_its_position_or_the_batch_size():
    emb, protos = _rows(257, 50), _unit32(_rows(300, 51))
    rng = np.random.Generator(np.random.PCG64(52))
    pclass, live = _dev(rng.integers(0, 40, size=300).astype(np.int32)), _dev((rng.uniform(size=300) > 0.2).astype(np.uint8))
    emb_d, protos_d = _dev(emb), _dev(protos)
    sc = dict(live=live, pclass=pclass, n_classes=40, scale=16.0, k=8)
    whole = _score(emb_d, protos_d, **sc)
    again = _score(emb_d, protos_d, **sc)
    assert _same_bits(whole, again, slice(None), slice(None))                      # the same call twice: the same bits
    for i in (0, 1, 2, 3, 100, 255, 256):
        alone = _score(emb_d[i:i + 1].clone(), protos_d, **sc)
        assert _same_bits(whole, alone, [i], [0]), i
        trio = _score(emb_d[[7, i, 200]].clone(), protos_d, **sc)
        assert _same_bits(whole, trio, [7, i, 200], [0, 1, 2]), i
    moved = _score(torch.roll(emb_d, 1, 0).clone(), protos_d, **sc)                 # every row in another slot of its workgroup
    assert _same_bits(whole, moved, np.arange(257), (np.arange(257) + 1) % 257)
    # batches large enough for the kernel to give a workgroup two and four rows (it picks by batch size): still the same bits
    for copies in (2, 4, 5):
        big = _score(emb_d.repeat(copies, 1)[1:].contiguous(), protos_d, **sc)        # (shifted by one: other slots again)
        rows = np.arange(257 * copies - 1)
        assert _same_bits(whole, big, (rows + 1) % 257, rows), copies


def test_identical_prototypes_in_two_classes_rank_the_lower_class_first():
    protos = _unit32(_rows(6, 60))
    protos[4] = protos[1]
    emb = np.stack([protos[1] * 2.5, protos[4] * 0.01, _rows(1, 61)[0]]).astype(np.float32)
    pclass = np.array([3, 5, 0, 1, 2, 4], np.int32)                   # the twins: prototype 1 in class 5, prototype 4 in class 2
    got = _score(_dev(emb), _dev(protos), pclass=_dev(pclass), n_classes=6, k=3)
    assert got["cls"][0, :2].tolist() == [2, 5] and got["cls"][1, :2].tolist() == [2, 5]
    assert got["sim"][0, 0] == got["sim"][0, 1] and got["prob"][0, 0] == got["prob"][0, 1]
    assert got["nearest"][0] == 4 and got["nearest"][1] == 4
    got = _score(_dev(emb), _dev(protos), k=2)                        # class = row: classes 1 and 4
    assert got["cls"][0].tolist() == [1, 4] and got["nearest"][0] == 1


def test_rows_that_cannot_be_scored_give_minus_one_and_nan():
    emb, protos = _rows(9, 70), _unit32(_rows(33, 71))
    clean = _score(_dev(emb), _dev(protos), scale=4.0, k=3)
    emb[1, 3] = np.nan
    emb[4, 511] = -np.inf
    emb[6] = 0.0
    got = _score(_dev(emb), _dev(protos), scale=4.0, k=3)
    bad, good = [1, 4, 6], [0, 2, 3, 5, 7, 8]
    assert (got["cls"][bad] == -1).all() and (got["nearest"][bad] == -1).all()
    assert np.isnan(got["sim"][bad]).all() and np.isnan(got["prob"][bad]).all() and np.isnan(got["sims"][bad]).all()
    assert _same_bits(got, clean, good, good)


# ---- 6. refused calls ------------------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing():
    lib, h, st, EINVAL = _lib(), _h(), _st(), _native.SIR_EINVAL
    P, B, k = 5, 4, 3
    nbytes = lib.sir_proto_state_bytes(P)
    assert lib.sir_proto_state_bytes(0) == 0 and lib.sir_proto_state_bytes(4097) == 0 and lib.sir_proto_state_bytes(4096) > 0
    state = _new_state(P)
    _accumulate(state, P, _rows(B, 80), [0, 1, 2, 3])
    state0 = state.clone()
    fresh = torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device=DEV)         # never reset: the header holds no n_classes
    emb, labels = _dev(_rows(B, 81)), torch.zeros(B, dtype=torch.int64, device=DEV)
    mask = torch.ones(P, dtype=torch.uint8, device=DEV)
    outs = {n: torch.full(shape, SENTINEL, dtype=torch.uint8, device=DEV) for n, shape in
            (("protos", (P * DIM * 4,)), ("live", (P,)), ("sims", (B * P * 4,)), ("cls", (B * k * 4,)), ("sim", (B * k * 4,)),
             ("prob", (B * k * 4,)), ("nearest", (B * 4,)))}
    o = {n: t.data_ptr() for n, t in outs.items()}
    sp, ep, lp = state.data_ptr(), emb.data_ptr(), labels.data_ptr()
    protos = _dev(_unit32(_rows(P, 82)))
    pp = protos.data_ptr()
    pclass = torch.zeros(P, dtype=torch.int32, device=DEV)
    refused = [
        # a required pointer is NULL
        lambda: lib.sir_proto_reset(None, sp, nbytes, P, None, st),
        lambda: lib.sir_proto_reset(h, None, nbytes, P, None, st),
        lambda: lib.sir_proto_accumulate(h, sp, nbytes, P, None, lp, B, st),
        lambda: lib.sir_proto_accumulate(h, sp, nbytes, P, ep, None, B, st),
        lambda: lib.sir_proto_finalize(h, sp, nbytes, P, None, o["live"], st),
        lambda: lib.sir_proto_finalize(h, sp, nbytes, P, o["protos"], None, st),
        lambda: lib.sir_proto_score(h, None, B, pp, None, None, P, P, None, k, o["sims"], o["cls"], o["sim"], o["prob"], o["nearest"], st),
        lambda: lib.sir_proto_score(h, ep, B, None, None, None, P, P, None, k, o["sims"], o["cls"], o["sim"], o["prob"], o["nearest"], st),
        lambda: lib.sir_proto_score(h, ep, B, pp, None, None, P, P, None, k, o["sims"], None, o["sim"], o["prob"], o["nearest"], st),
        lambda: lib.sir_proto_score(h, ep, B, pp, None, None, P, P, None, k, o["sims"], o["cls"], None, o["prob"], o["nearest"], st),
        lambda: lib.sir_proto_score(h, ep, B, pp, None, None, P, P, None, k, o["sims"], o["cls"], o["sim"], None, o["nearest"], st),
        # a count outside its range
        lambda: lib.sir_proto_reset(h, sp, nbytes, 0, None, st),
        lambda: lib.sir_proto_reset(h, sp, nbytes, 4097, None, st),
        lambda: lib.sir_proto_accumulate(h, sp, nbytes, P, ep, lp, 0, st),
        lambda: lib.sir_proto_accumulate(h, sp, nbytes, 0, ep, lp, B, st),
        lambda: lib.sir_proto_finalize(h, sp, nbytes, 4097, o["protos"], o["live"], st),
        lambda: lib.sir_proto_score(h, ep, 0, pp, None, None, P, P, None, k, o["sims"], o["cls"], o["sim"], o["prob"], o["nearest"], st),
        lambda: lib.sir_proto_score(h, ep, B, pp, None, None, 0, 1, None, k, o["sims"], o["cls"], o["sim"], o["prob"], o["nearest"], st),
        lambda: lib.sir_proto_score(h, ep, B, pp, None, None, 4097, P, None, k, o["sims"], o["cls"], o["sim"], o["prob"], o["nearest"], st),
        lambda: lib.sir_proto_score(h, ep, B, pp, None, pclass.data_ptr(), P, 0, None, k, o["sims"], o["cls"], o["sim"], o["prob"], o["nearest"], st),
        lambda: lib.sir_proto_score(h, ep, B, pp, None, pclass.data_ptr(), P, P + 1, None, k, o["sims"], o["cls"], o["sim"], o["prob"], o["nearest"], st),
        lambda: lib.sir_proto_score(h, ep, B, pp, None, None, P, P - 1, None, k, o["sims"], o["cls"], o["sim"], o["prob"], o["nearest"], st),
        # k
        lambda: lib.sir_proto_score(h, ep, B, pp, None, None, P, P, None, 9, o["sims"], o["cls"], o["sim"], o["prob"], o["nearest"], st),
        lambda: lib.sir_proto_score(h, ep, B, pp, None, None, P, P, None, 0, o["sims"], o["cls"], o["sim"], o["prob"], o["nearest"], st),
        # state_bytes too small
        lambda: lib.sir_proto_reset(h, sp, nbytes - 1, P, None, st),
        lambda: lib.sir_proto_accumulate(h, sp, nbytes - 1, P, ep, lp, B, st),
        lambda: lib.sir_proto_finalize(h, sp, nbytes - 1, P, o["protos"], o["live"], st),
        # the header's n_classes disagrees with the argument
        lambda: lib.sir_proto_accumulate(h, sp, nbytes, P - 1, ep, lp, B, st),
        lambda: lib.sir_proto_finalize(h, sp, nbytes, P - 1, o["protos"], o["live"], st),
        lambda: lib.sir_proto_reset(h, sp, nbytes, P - 1, mask.data_ptr(), st),
        lambda: lib.sir_proto_accumulate(h, fresh.data_ptr(), nbytes, P, ep, lp, B, st),
        lambda: lib.sir_proto_finalize(h, fresh.data_ptr(), nbytes, P, o["protos"], o["live"], st),
        lambda: lib.sir_proto_reset(h, fresh.data_ptr(), nbytes, P, mask.data_ptr(), st),
    ]
    for i, call in enumerate(refused):
        assert call() == EINVAL, (i, lib.sir_last_error())
        assert lib.sir_last_error()
    torch.cuda.synchronize()
    assert torch.equal(state, state0) and (fresh == SENTINEL).all()
    for n, t in outs.items():
        assert (t == SENTINEL).all(), n
    # sir_model_embed: emb is required, argmax needs logits
    sd = synth.synth_state_dict(31, seed=0)
    m = _model(sd)
    x = synth.synth_features(2, 16, seed=1).to(DEV)
    ops.model_embed(m, x, m._ws)                                      # (sizes the workspace and caches the weights)
    w, keep = ops.cached_weights(m)
    ws = m._ws.buf
    amax = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    assert lib.sir_model_embed(h, C.byref(w), x.data_ptr(), None, 2, 16, None, None, None, ws.data_ptr(), ws.numel(), st) == EINVAL
    assert lib.sir_model_embed(h, C.byref(w), x.data_ptr(), None, 2, 16, o["protos"], None, amax.data_ptr(), ws.data_ptr(), ws.numel(),
                               st) == EINVAL
    torch.cuda.synchronize()
    assert (amax == -7).all() and (outs["protos"] == SENTINEL).all()
    ops.check_status()


# ---- 7. surface ------------------------------------------------------------------------------------------------------------
INTENTS = ["lights_on", "lights_off", "volume_up", "volume_down", "heat_up", "heat_down"]


@pytest.fixture(scope="module")
def enrolled(sd):
    """six feature clips as six intents, each enrolled from five slightly noised copies; fresh copies to score"""
    m = _model(sd)
    base = synth.synth_features(6, 200, seed=90)
    g = torch.Generator().manual_seed(91)
    noisy = lambda n: (base.repeat_interleave(n, 0) + 0.02 * torch.randn(6 * n, 64, 200, generator=g)).to(DEV)
    train, fresh = m.embed(noisy(5)), m.embed(noisy(2))
    names = [n for n in INTENTS for _ in range(5)]
    bank = PrototypeBank().enroll(train, names)
    return {"model": m, "bank": bank, "train": train, "names": names, "fresh": fresh, "truth": [n for n in INTENTS for _ in range(2)]}


def test_bank_scores_and_result_dictionaries(enrolled):
    from sir_amd.scripts import classify_results
    bank, fresh, truth = enrolled["bank"], enrolled["fresh"], enrolled["truth"]
    assert bank.names == INTENTS and bank.state_arrays()["count"].tolist() == [5] * 6 and bank.state_arrays()["skipped"] == 0
    s = bank.score(fresh, k=3, scale=16.0, min_similarity=0.5)
    assert [INTENTS[c] for c in s.classes[:, 0].tolist()] == truth
    assert (s.nearest == s.classes[:, 0]).all() and s.rejected.dtype == torch.bool
    protos, live, pclass = bank.prototypes()
    assert pclass is None and live.all() and bank.prototypes()[0] is protos         # cached until the bank changes
    ref = proto_ref.score(fresh.cpu().numpy(), protos.cpu().numpy(), scale=16.0)
    for b in range(12):
        assert proto_ref.check_ranking(ref["s"][b], s.classes[b].cpu().numpy(), 3) is None
    res = classify_results.results_from_prototypes(fresh, bank, k=3, scale=16.0, min_similarity=0.5)
    for b, r in enumerate(res):
        assert r["predicted_label"] == truth[b] == r["top_predictions"][0]["label"] and len(r["top_predictions"]) == 3
        assert r["confidence"] == float(s.probs[b, 0]) == r["top_predictions"][0]["probability"]
        assert r["similarity"] == float(s.sims[b, 0]) and r["nearest"] == int(s.nearest[b])
        assert r["rejected"] == bool(s.rejected[b]) == (not r["similarity"] >= 0.5)
    assert all(r["rejected"] for r in classify_results.results_from_prototypes(fresh, bank, min_similarity=2.0))
    assert not any(r["rejected"] for r in classify_results.results_from_prototypes(fresh, bank, min_similarity=-2.0))
    assert "rejected" not in classify_results.results_from_prototypes(fresh, bank)[0]
    # the bank's own scale is the default; fit_scale gives one from a labelled split
    beta = fit_scale(bank, enrolled["train"], torch.tensor([INTENTS.index(n) for n in enrolled["names"]], device=DEV))
    assert 1.0 / 64 <= float(beta[0]) <= 64.0
    bank.scale = 16.0
    assert torch.equal(bank.score(fresh).probs, s.probs)
    bank.scale = None
    # a removed class is absent until it is enrolled again
    bank.remove("volume_up")
    s2 = bank.score(fresh, k=8)
    assert not (s2.classes == 2).any() and (s2.classes[:, 5:] == -1).all() and (s2.classes[:, :5] >= 0).all()
    bank.enroll(enrolled["train"][10:15], ["volume_up"] * 5)
    assert torch.equal(bank.score(fresh, k=3, scale=16.0).classes, s.classes)


def test_save_load_enroll_continues_to_the_same_bits(enrolled, tmp_path):
    train, names = enrolled["train"], enrolled["names"]
    order = np.random.Generator(np.random.PCG64(92)).permutation(30).tolist()      # classes interleaved, new names arriving late
    rows, labels = train[order], [names[i] for i in order]
    whole = PrototypeBank().enroll(rows, labels)
    part = PrototypeBank().enroll(rows[:13], labels[:13])
    part.save(str(tmp_path / "bank.npz"))
    back = PrototypeBank.load(str(tmp_path / "bank.npz")).enroll(rows[13:], labels[13:])
    a, b = whole.state_arrays(), back.state_arrays()
    assert whole.names == back.names
    assert np.array_equal(a["sum"], b["sum"]) and np.array_equal(a["count"], b["count"]) and a["skipped"] == b["skipped"] == 0
    assert torch.equal(whole.prototypes()[0], back.prototypes()[0])


def test_exemplars_with_one_row_per_class_reproduce_the_mean_bank(enrolled):
    train, fresh = enrolled["train"], enrolled["fresh"]
    rows = train[::5]                                                 # one example per class
    mean = PrototypeBank().enroll(rows, INTENTS)
    ex = PrototypeBank(exemplars=True).enroll(rows, INTENTS)
    assert torch.equal(mean.prototypes()[0], ex.prototypes()[0]) and ex.prototypes()[2].tolist() == list(range(6))
    a, b = mean.score(fresh, k=6, scale=8.0), ex.score(fresh, k=6, scale=8.0)
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(x, y)
    # all thirty rows as exemplars: 1-NN; a class named but never enrolled stays absent
    nn = PrototypeBank(["never_enrolled"] + INTENTS, exemplars=True).enroll(train, enrolled["names"])
    s = nn.score(fresh, k=8)
    assert [nn.names[c] for c in s.classes[:, 0].tolist()] == enrolled["truth"]
    assert (s.classes[:, 6:] == -1).all() and not (s.classes == 0).any()
    assert all(nn._row_class[r] == c for r, c in zip(s.nearest.tolist(), s.classes[:, 0].tolist()))
    with pytest.raises(_native.SirError, match="at most 4096 rows"):
        PrototypeBank(exemplars=True).enroll(torch.ones((4097, DIM), device=DEV), ["a"] * 4097)


def test_predict_many_with_prototypes(enrolled, tmp_path):
    from sir_amd.scripts import classify_results, predict_frontend, test_model
    from sir_amd.scripts.utils import wav_io
    m, bank = enrolled["model"], enrolled["bank"]
    clips = synth.synth_clips(3, 40000, seed=93)
    paths = []
    for i in range(3):
        paths.append(str(tmp_path / f"utt{i}.wav"))
        wav_io.write_wav_pcm16(paths[-1], clips[i], 16000)
    paths.insert(1, str(tmp_path / "missing.wav"))
    res = predict_frontend.predict_many(m, paths, {}, torch.device(DEV), prototypes=bank, min_similarity=0.3)
    assert res[1] is None and all(r is not None for r in res[:1] + res[2:])
    feats = predict_frontend.get_extractor().extract_batch([p for p in paths if "missing" not in p], max_duration=600.0)
    batch = torch.stack([test_model._pad_or_trim(f.unsqueeze(0), 200)[0] for f in feats]).to(DEV)
    want = classify_results.results_from_prototypes(m.embed(batch), bank, min_similarity=0.3)
    assert [r for r in res if r is not None] == want
    assert all(r["predicted_label"] in INTENTS and "rejected" in r and -1.0 <= r["similarity"] <= 1.0 for r in want)
    ops.check_status()


def test_recordings_and_streams_with_prototypes(enrolled):
    from sir_amd.scripts import classify_results
    from sir_amd.scripts.testing import IntentRecognizer
    m, bank = enrolled["model"], enrolled["bank"]
    utt = synth.synth_clips(4, 40000, seed=77).numpy()
    z = lambda chunks: np.zeros(chunks * 1024, dtype=np.float32)
    recs = [np.concatenate([z(8), utt[0, :24 * 1024], z(24), utt[1, :32 * 1024], z(20)]),
            np.concatenate([utt[2, :16 * 1024], z(32), utt[3, :5 * 1024], z(8)])]
    reco = IntentRecognizer.from_model(m, {f"intent_{i}": i for i in range(31)}, DEV)
    want = reco.recognize_recordings(recs, pad_to=200, prototypes=bank, min_similarity=0.3)
    assert [len(f) for f in want] == [2, 2]
    wave, wl = reco._load_group(recs)
    _, emb = reco.score_segments(wave, wl, pad_to=200, logits_on_device=True, embed=True)
    direct = classify_results.results_from_prototypes(emb, bank, min_similarity=0.3)
    flat_want = [w for f in want for w in f]
    assert [{k: v for k, v in w.items() if k not in ("start", "end")} for w in flat_want] == direct
    assert all(all(r["rejected"] for r in f) for f in reco.recognize_recordings(recs, pad_to=200, prototypes=bank, min_similarity=2.0))
    assert not any(r["rejected"] for f in reco.recognize_recordings(recs, pad_to=200, prototypes=bank, min_similarity=-2.0) for r in f)
    # a stream yields what recognize_recordings gives on the whole recording
    session = reco.open_streams(2, max_push=1000, pad_to=200, prototypes=bank, min_similarity=0.3)
    found, embs = [[], []], [[], []]
    for k in range(-(-max(len(r) for r in recs) // 1000)):
        chunks = {s: r[k * 1000:(k + 1) * 1000] for s, r in enumerate(recs) if k * 1000 < len(r)}
        close = [s for s, r in enumerate(recs) if k * 1000 < len(r) <= (k + 1) * 1000]
        for row, u in enumerate(session.feed(chunks, close=close)):
            found[u["stream"]].append(u)
            embs[u["stream"]].append(session.last_logits[row])
    flat = [u for f in found for u in f]
    assert len(flat) == 4
    for u, w in zip(flat, flat_want):
        assert u["forced"] is False and {k: v for k, v in u.items() if k not in ("stream", "forced")} == w
    assert torch.equal(torch.stack([e for rows in embs for e in rows]), emb)
    ops.check_status()


def test_enroll_script_and_the_evaluate_key(enrolled, tmp_path):
    from sir_amd.scripts import enroll, evaluate, predict_frontend
    from sir_amd.scripts.utils import wav_io
    clips = synth.synth_clips(5, 30000, seed=95)
    rows = []
    for i in range(5):
        path = str(tmp_path / f"ex{i}.wav")
        wav_io.write_wav_pcm16(path, clips[i], 16000)
        rows.append((path, ["door_open", "door_close"][i % 2]))
    rows.append((str(tmp_path / "missing.wav"), "door_open"))
    with open(tmp_path / "examples.csv", "w") as f:
        f.write("path,label\n" + "".join(f"{p},{label}\n" for p, label in rows))
    sd = synth.synth_state_dict(31, seed=0)
    torch.save(sd, str(tmp_path / "model.pt"))
    common = ["--checkpoint", str(tmp_path / "model.pt"), "--exemplars", "--batch_size", "4"]
    assert enroll.main(["--csv", str(tmp_path / "examples.csv"), "--out", str(tmp_path / "bank.npz")] + common) == 0
    bank = PrototypeBank.load(str(tmp_path / "bank.npz"))
    assert bank.names == ["door_open", "door_close"] and bank.exemplars and bank._row_class == [0, 1, 0, 1, 0]
    # every enrolled file is its own nearest exemplar at cosine 1: enrolment and scoring see the same function
    res = predict_frontend.predict_many(enrolled["model"], [p for p, _ in rows[:5]], {}, torch.device(DEV), prototypes=bank)
    assert [r["predicted_label"] for r in res] == [label for _, label in rows[:5]] and [r["nearest"] for r in res] == [0, 1, 2, 3, 4]
    assert all(abs(r["similarity"] - 1.0) <= SIM_BOUND for r in res)
    # --append continues the file: two more examples of a new class
    with open(tmp_path / "more.csv", "w") as f:
        f.write(f"{rows[0][0]},window_open\n{rows[1][0]},window_open\n")
    assert enroll.main(["--csv", str(tmp_path / "more.csv"), "--append", str(tmp_path / "bank.npz"), "--out", str(tmp_path / "bank2.npz")]
                       + common) == 0
    bank2 = PrototypeBank.load(str(tmp_path / "bank2.npz"))
    assert bank2.names == ["door_open", "door_close", "window_open"] and bank2.n_rows == 7
    assert np.array_equal(bank2.state_arrays()["sum"][:5], bank.state_arrays()["sum"])
    # evaluate.py's `prototypes:` key: both heads' top-1 / top-3 from the same forward passes
    feats = predict_frontend.get_extractor().extract_batch([p for p, _ in rows[:5]], max_duration=600.0)
    from sir_amd.scripts import test_model
    mel = torch.stack([test_model._pad_or_trim(f.unsqueeze(0), 200)[0] for f in feats])
    inv = {0: "door_open", 1: "door_close", 2: "never_enrolled"}
    loader = [(mel[:3], torch.tensor([0, 1, 0])), (None, None), (mel[3:], torch.tensor([1, 2]))]
    out = evaluate.prototype_metrics_file(enrolled["model"], loader, torch.device(DEV), str(tmp_path / "bank.npz"), inv,
                                          str(tmp_path / "results" / "prototype_metrics.json"))
    assert out["n"] == 5 and out["n_unknown"] == 1 and out["prototypes"] == {"top1": 0.8, "top3": 0.8}
    assert 0.0 <= out["fc"]["top1"] <= out["fc"]["top3"] <= 1.0
    import json
    assert json.load(open(tmp_path / "results" / "prototype_metrics.json")) == out
    ops.check_status()
