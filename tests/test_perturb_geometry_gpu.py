"""GPU: ``sir_wave_perturb`` at every WSOLA geometry its entry point accepts, at its store paths and at its range edges,
against the float64 contract of tests/wave_perturb_ref.py (the method of tests/test_wave_perturb_gpu.py: read the offsets
the kernel chose through ``offsets_out`` and rebuild each pass in float64 from them).

Sample rates and geometries (S, W, O, H) covered here; 16 000 Hz (1312, 235, 192, 1120) is test_wave_perturb_gpu.py's:

    8 000   (656, 117,  96,  560)   W < 128: waves 2 and 3 carry only the sentinel into the argmin's LDS merge
    8 500   (697, 125, 104,  593)   H odd: scalar stores everywhere, unaligned segment bases
   11 025   (904, 162, 136,  768)
   22 050  (1808, 324, 264, 1544)   W > 256: a thread owns two candidates
   24 000  (1968, 352, 288, 1680)   W + S = 2320 of the 2368-sample LDS window, O = 288 = the LDS tail, all ten prefetch registers

Rows per rate: max_len = 2 sr, lengths [2 sr, 0, 1, W/2, H-1, H, H+1, S, 2H, 3H+7, 2 sr - 1], float32 and int16; tempo
0.5 / 0.7 / 0.85 / 1.15 / 1.5 / 2 and a per-row draw from [0.5, 2]; cents -200 / -37.5 / 150 / 200; one shifted
pitch-then-speed batch.  Tolerances are the project's: offset slack 1e-4 relative, samples
1e-6 max|x| (tempo), 2e-6 (pitch), 4e-6 (chain), the float64 argmin on >= 99 % of the segments of each test.

Exact ties (a burst followed by zeros, an all-zero clip): the kernel must pick the FIRST minimum -- inside a thread that
owns two candidates, across the wave shuffle and across the four wave leaders -- which the slack rule alone cannot see.

Store paths: the 16-byte (float4) store branch of the tempo pass into the caller's buffer is pinned bit for bit to the
scalar branch (odd row stride, and a base pointer that is not 16-byte aligned): the scalar branch is the one the float64
comparisons of test_wave_perturb_gpu.py go through (HipFeaturizer.perturb's default ``max_out_len`` is odd there), the
float4 branch the one the tempo comparisons above go through wherever H % 4 == 0 (their ``max_out_len`` is a multiple of 4).
A ``max_out_len`` that cuts the output leaves the prefix bit-identical, writes every element of [0, max_out_len) and
nothing behind it.

Range edges (16 kHz handle): tempo 0.5 / 2 and cents +-200 are accepted, the next float32 beyond them, NaN and tempo 0
zero their own row only (length 0, whichever pass of a pitch-then-speed call rejects it) and are reported once by
``check_status``; lengths are clamped to [0, max_len]; handles at 7 999
and 24 001 Hz are created by ``sir_create_ex`` (it takes any positive rate) and refused by ``sir_wave_perturb`` itself with
SIR_EUNSUPPORTED before it touches ``out``."""
import numpy as np
import pytest
import torch

import perturb_geometry_cases as cases
import wave_perturb_ref as ref
from oracle import features_ref
from sir_amd import _native, ops, synth
from sir_amd.featurizer import HipFeaturizer, get_featurizer
from test_wave_perturb_gpu import _Tally

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0                  # no sample of a clip in [-1, 1] comes out as this


def _status(fz):
    """sir_check_status on this handle (ops.check_status reads the default 16 kHz handle's status word)."""
    torch.cuda.synchronize()
    _native.check(_native.lib().sir_check_status(fz.handle, _native.current_stream_ptr()), "sir_check_status")


def _dev(t, dtype):
    return None if t is None else torch.as_tensor(t).to(device="cuda", dtype=dtype).contiguous()


def _call(fz, x, lens, max_out_len, shift=None, cents=None, tempo=None, max_seg=None):
    """HipFeaturizer.perturb with the offsets hook -> (out, out_len, offsets) on the host, status checked."""
    max_seg = cases.max_segments(fz.sample_rate) if max_seg is None else max_seg
    offs = torch.full((x.shape[0], 2, max_seg), 7, dtype=torch.int32, device="cuda")
    out, out_len = fz.perturb(x.cuda(), _dev(lens, torch.int32), shift=_dev(shift, torch.int32),
                              pitch_cents=_dev(cents, torch.float32), tempo=_dev(tempo, torch.float32),
                              max_out_len=max_out_len, offsets_out=offs)
    _status(fz)
    return out.cpu(), out_len.cpu(), offs.cpu().numpy()


def _raw(fz, x, lens, max_out_len, out_stride, tempo=None, cents=None, lead=0, check=True):
    """sir_wave_perturb through ctypes into a SENTINEL-filled buffer whose first row starts ``lead`` floats into a
    16-byte-aligned allocation -> (rc, out [B, out_stride] on the host, out_len, offsets)."""
    lib = _native.lib()
    bsz, max_len = x.shape
    xd, ld = x.cuda().contiguous(), _dev(lens, torch.int32)
    td, cd = _dev(tempo, torch.float32), _dev(cents, torch.float32)
    buf = torch.full((lead + bsz * out_stride + 4,), SENTINEL, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0 and out_stride >= max_out_len
    out_len = torch.full((bsz,), -7, dtype=torch.int32, device="cuda")
    max_seg = cases.max_segments(fz.sample_rate)
    offs = torch.full((bsz, 2, max_seg), 7, dtype=torch.int32, device="cuda")
    ws, nbytes = None, 0
    if cents is not None:
        nbytes = lib.sir_perturb_workspace_bytes(fz.handle, bsz, max_len)
        wst = torch.empty(nbytes + 256, dtype=torch.uint8, device="cuda")
        ws = (wst.data_ptr() + 255) // 256 * 256
    dt = {torch.float32: _native.WAVE_F32, torch.int16: _native.WAVE_I16}[x.dtype]
    rc = lib.sir_wave_perturb(fz.handle, xd.data_ptr(), dt, xd.stride(0), ld.data_ptr(), bsz, max_len, None,
                              cd.data_ptr() if cd is not None else None, td.data_ptr() if td is not None else None,
                              buf.data_ptr() + 4 * lead, out_stride, max_out_len, out_len.data_ptr(), offs.data_ptr(), max_seg,
                              ws, nbytes, _native.current_stream_ptr())
    torch.cuda.synchronize()
    if check:
        _native.check(rc, "sir_wave_perturb")
        _status(fz)
    whole = buf.cpu()
    assert (whole[:lead] == SENTINEL).all() and (whole[lead + bsz * out_stride:] == SENTINEL).all()
    return rc, whole[lead:lead + bsz * out_stride].view(bsz, out_stride), out_len.cpu(), offs.cpu().numpy()


def _scale(xb):
    return max(np.abs(xb).max(initial=0.0), 1e-30)


def _full_len(sr):
    """max_out_len that truncates no row of the tests: 2 max_len + 4, rounded up to a multiple of 4."""
    return cases.round_up4(2 * (2 * sr) + 4)


# ---- 1. every geometry against the float64 contract -------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.int16], ids=["f32", "i16"])
@pytest.mark.parametrize("sr", cases.RATES)
def test_tempo_matches_float64_contract(sr, dtype):
    S, W, O, H = ref.geometry(sr)
    assert (S, W, O, H) == cases.GEOMETRY[sr]
    fz = get_featurizer(sr)
    lens = cases.lengths_for(sr)
    x = cases.clips(sr, dtype)
    xs = [cases.host_f64(x, b, n) for b, n in enumerate(lens)]
    lib = _native.lib()
    tally = _Tally()
    factors = [np.full(len(lens), f, dtype=np.float32) for f in cases.TEMPO_FACTORS] + [cases.per_row_factors(len(lens))]
    for fs in factors:
        out, out_len, offs = _call(fz, x, lens, _full_len(sr), tempo=fs)
        assert out.shape[1] == _full_len(sr) and (offs[:, 0] == -1).all()
        for b, n in enumerate(lens):
            f = float(fs[b])
            want_len = ref.out_len(n, f)
            assert int(out_len[b]) == want_len == lib.sir_perturb_out_len(n, f), (b, f)
            y, used, costs = ref.tempo(xs[b], f, sr, offsets=offs[b, 1])
            assert len(used) == int((offs[b, 1] >= 0).sum()) == -(-want_len // H), (b, f)
            tally.check_pass(offs[b, 1], costs)
            got = out[b].double().numpy()
            err = np.abs(got[:want_len] - y).max(initial=0.0) / _scale(xs[b])
            assert err <= 1e-6, (sr, b, f, err)
            assert (got[want_len:] == 0).all(), (b, f)
    tally.check_rate()


@pytest.mark.parametrize("dtype", [torch.float32, torch.int16], ids=["f32", "i16"])
@pytest.mark.parametrize("sr", cases.RATES)
def test_pitch_matches_float64_contract(sr, dtype):
    fz = get_featurizer(sr)
    lens = cases.lengths_for(sr)
    x = cases.clips(sr, dtype)
    xs = [cases.host_f64(x, b, n) for b, n in enumerate(lens)]
    tally = _Tally()
    for c in cases.PITCH_CENTS:
        out, out_len, offs = _call(fz, x, lens, 2 * sr, cents=np.full(len(lens), c, dtype=np.float32))
        assert (offs[:, 1] == -1).all()
        d = 2.0 ** (c / 1200.0)
        for b, n in enumerate(lens):
            assert int(out_len[b]) == n
            s, used, costs = ref.tempo(xs[b], 1.0 / d, sr, offsets=offs[b, 0])
            assert len(s) == ref.out_len(n, 1.0 / d) and len(used) == int((offs[b, 0] >= 0).sum()), (b, c)
            tally.check_pass(offs[b, 0], costs)
            y = ref.resample_frac(s, d, n)
            got = out[b].double().numpy()
            err = np.abs(got[:n] - y).max(initial=0.0) / _scale(xs[b])
            assert err <= 2e-6, (sr, b, c, err)
            assert (got[n:] == 0).all(), (b, c)
    tally.check_rate()


@pytest.mark.parametrize("sr", cases.RATES)
def test_chain_pitch_then_speed(sr):
    """Shifted rows, pitch then speed, every row against the float64 chain; two calls give the same bits (at 8 500 Hz the
    pitch pass writes its workspace with scalar stores at unaligned segment bases)."""
    fz = get_featurizer(sr)
    lens = cases.lengths_for(sr)
    x = cases.clips(sr)
    rng = np.random.default_rng(sr)
    shift = np.array([int(rng.integers(-n // 10, n // 10 + 1)) or 3 for n in lens], dtype=np.int32)
    cents = rng.uniform(-200.0, 200.0, len(lens)).astype(np.float32)
    tempo = rng.uniform(0.5, 2.0, len(lens)).astype(np.float32)
    assert (shift != 0).all() and (cents != 0).all() and (tempo != 1).all()
    first = _call(fz, x, lens, _full_len(sr), shift=shift, cents=cents, tempo=tempo)
    again = _call(fz, x, lens, _full_len(sr), shift=shift, cents=cents, tempo=tempo)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1]) and np.array_equal(first[2], again[2])
    out, out_len, offs = first
    for b, n in enumerate(lens):
        xsh = ref.shifted(cases.host_f64(x, b, n), int(shift[b]))
        y, _, _, _ = ref.pitch(xsh, float(cents[b]), sr, offsets=offs[b, 0])
        z, _, _ = ref.tempo(y, float(tempo[b]), sr, offsets=offs[b, 1])
        m = int(out_len[b])
        assert m == len(z) == ref.out_len(n, float(tempo[b])), b
        got = out[b].double().numpy()
        err = np.abs(got[:m] - z).max(initial=0.0) / _scale(xsh)
        assert err <= 4e-6, (sr, b, err)
        assert (got[m:] == 0).all(), b


@pytest.mark.parametrize("sr", [8000, 16000, 22050, 24000])
def test_first_minimum_on_exact_ties(sr):
    """Candidates whose cost is the same float exactly: the kernel's offset IS the first of them.  At 22 050 and 24 000 Hz
    candidates i and i + 256 belong to one thread; lanes of one wave and the four wave leaders tie as well."""
    S, W, O, H = ref.geometry(sr)
    fz = get_featurizer(sr)
    firsts = sorted({0, 1, 40, 63, 64, 65, 100, min(200, W - 2), W - 1})
    n = 8 * H                                                            # 16 segments at tempo 0.5
    x = torch.stack([torch.zeros(n)] + [cases.tie_clip(sr, a, n) for a in firsts[1:]])
    out, out_len, offs = _call(fz, x, [n] * len(firsts), 2 * n + 4, tempo=np.full(len(firsts), 0.5, dtype=np.float32))
    for b, a in enumerate(firsts):
        xb = x[b].double().numpy()
        y, used, costs = ref.tempo(xb, 0.5, sr)
        assert int(out_len[b]) == 2 * n and len(used) == 16
        assert used == [W // 2, a] + [0] * 14 and (costs[0][a:] == 0).all() and (costs[0][:a] > 0).all()
        assert offs[b, 1, :16].tolist() == used, (sr, a, offs[b, 1, :4].tolist())
        assert (offs[b, 1, 16:] == -1).all()
        assert np.abs(out[b, :2 * n].double().numpy() - y).max() <= 1e-6 * _scale(xb)
    # the same at tempo 2 and through the pitch pass, on the all-zero clip: every later offset is 0
    zero = torch.zeros(1, 2 * sr)
    _, n2, o2 = _call(fz, zero, [2 * sr], _full_len(sr), tempo=np.float32([2.0]))
    assert int(n2[0]) == sr and o2[0, 1, :-(-sr // H)].tolist() == [W // 2] + [0] * (-(-sr // H) - 1)
    _, n3, o3 = _call(fz, zero, [2 * sr], 2 * sr, cents=np.float32([-200.0]))
    ns = -(-ref.out_len(2 * sr, 2.0 ** (200.0 / 1200.0)) // H)
    assert int(n3[0]) == 2 * sr and o3[0, 0, :ns].tolist() == [W // 2] + [0] * (ns - 1) and (o3[0, 0, ns:] == -1).all()


# ---- 2. store paths and truncation -------------------------------------------------------------------------------------

@pytest.mark.parametrize("sr", [8000, 16000, 24000])
def test_vector_stores_match_scalar_stores_bit_for_bit(sr):
    S, W, O, H = ref.geometry(sr)
    assert H % 4 == 0
    fz = get_featurizer(sr)
    lens = cases.lengths_for(sr)
    x = cases.clips(sr)
    tempo = cases.per_row_factors(len(lens), seed=11)
    tempo[:3] = [0.5, 0.7, 2.0]
    M = _full_len(sr)
    assert M % 4 == 0 and all(ref.out_len(n, float(f)) <= M for n, f in zip(lens, tempo))
    _, vec, vec_len, vec_offs = _raw(fz, x, lens, M, M, tempo=tempo)                    # aligned base, stride % 4 == 0: float4
    _, odd, odd_len, odd_offs = _raw(fz, x, lens, M + 1, M + 1, tempo=tempo)            # odd stride: scalar
    _, mis, mis_len, mis_offs = _raw(fz, x, lens, M, M, tempo=tempo, lead=1)            # base 4 bytes off: scalar
    for got, got_len, got_offs in ((odd[:, :M], odd_len, odd_offs), (mis, mis_len, mis_offs)):
        assert torch.equal(vec.view(torch.int32), got.contiguous().view(torch.int32))
        assert torch.equal(vec_len, got_len) and np.array_equal(vec_offs, got_offs)
    assert (odd[:, M] == 0).all()                                                       # column M of the wider call is past every row
    assert [int(v) for v in vec_len] == [ref.out_len(n, float(f)) for n, f in zip(lens, tempo)]
    # and the float4 branch is what HipFeaturizer.perturb takes with an aligned max_out_len
    out, out_len, offs = _call(fz, x, lens, M, tempo=tempo)
    assert torch.equal(out.view(torch.int32), vec.contiguous().view(torch.int32)) and np.array_equal(offs, vec_offs)


@pytest.mark.parametrize("sr", [16000, 22050])
def test_truncation_by_max_out_len(sr):
    S, W, O, H = ref.geometry(sr)
    fz = get_featurizer(sr)
    lens = cases.lengths_for(sr)
    x = cases.clips(sr)
    tempo = np.full(len(lens), 0.7, dtype=np.float32)
    M = _full_len(sr)
    _, full, full_len, full_offs = _raw(fz, x, lens, M, M, tempo=tempo)
    for cap in (H - 1, H, H + 1, 2 * H, 2 * H + 3):
        stride = cases.round_up4(cap) + 8                                # aligned rows: whole segments go out as float4
        _, out, out_len, offs = _raw(fz, x, lens, cap, stride, tempo=tempo)
        assert (out[:, :cap] != SENTINEL).all() and (out[:, cap:] == SENTINEL).all(), cap
        for b, n in enumerate(lens):
            m = min(int(full_len[b]), cap)
            assert int(out_len[b]) == m == min(ref.out_len(n, float(tempo[b])), cap), (cap, b)
            assert torch.equal(out[b, :m].view(torch.int32), full[b, :m].view(torch.int32)), (cap, b)
            assert (out[b, m:cap] == 0).all(), (cap, b)
            nseg = -(-m // H)
            assert np.array_equal(offs[b, 1, :nseg], full_offs[b, 1, :nseg]) and (offs[b, 1, nseg:] == -1).all(), (cap, b)
            assert (offs[b, 0] == -1).all()


# ---- 3. range edges (16 kHz handle) ------------------------------------------------------------------------------------

SR16 = 16000


def _f32(v):
    return np.float32(v)


def _bad_rows_are_isolated(kind, good, bad_values):
    """``good``: a float32 factor per row, all accepted.  Each bad value replaces row 0's factor: that row is zeroed with
    out_len 0 and reported once; every other row keeps the bits of the all-good call."""
    fz = get_featurizer()
    lens = cases.lengths_for(SR16)
    x = cases.clips(SR16)
    M = _full_len(SR16) if kind == "tempo" else 2 * SR16
    base_out, base_len, base_offs = _call(fz, x, lens, M, **{kind: good})
    ops.check_status()
    for v in bad_values:
        fs = good.copy()
        fs[0] = v
        offs = torch.full((len(lens), 2, cases.max_segments(SR16)), 7, dtype=torch.int32, device="cuda")
        out, out_len = fz.perturb(x.cuda(), _dev(lens, torch.int32), max_out_len=M, offsets_out=offs,
                                  **{"pitch_cents" if kind == "cents" else "tempo": _dev(fs, torch.float32)})
        with pytest.raises(_native.SirError):
            ops.check_status()
        ops.check_status()                                              # the check that raised cleared the flag
        out, out_len, offs = out.cpu(), out_len.cpu(), offs.cpu().numpy()
        assert int(out_len[0]) == 0 and (out[0] == 0).all() and (offs[0] == -1).all(), v
        assert torch.equal(out[1:].view(torch.int32), base_out[1:].view(torch.int32)), v
        assert torch.equal(out_len[1:], base_len[1:]) and np.array_equal(offs[1:], base_offs[1:]), v
    return base_out, base_len, base_offs


def test_tempo_range_edges():
    lens = cases.lengths_for(SR16)
    good = np.float32([2.0, 0.5, 2.0, 0.5, 2.0, 0.5, 2.0, 0.5, 2.0, 0.5, 2.0])
    bad = [np.nextafter(_f32(0.5), _f32(0)), np.nextafter(_f32(2), _f32(3)), _f32("nan"), _f32(0)]
    assert bad[0] < 0.5 and bad[1] > 2.0
    out, out_len, offs = _bad_rows_are_isolated("tempo", good, bad)
    assert [int(v) for v in out_len] == [ref.out_len(n, float(f)) for n, f in zip(lens, good)]


def test_cents_range_edges():
    lens = cases.lengths_for(SR16)
    good = np.float32([200.0, -200.0] * 5 + [200.0])
    bad = [np.nextafter(_f32(200), _f32(300)), np.nextafter(_f32(-200), _f32(-300)), _f32("nan")]
    assert bad[0] > 200.0 and bad[1] < -200.0
    out, out_len, offs = _bad_rows_are_isolated("cents", good, bad)
    assert [int(v) for v in out_len] == lens


def test_bad_factor_in_the_chain_zeroes_its_row_whichever_pass_rejects_it():
    """Pitch then speed in one call: a row with bad cents and a good tempo, and one with good cents and a bad tempo, both
    come out zeroed with length 0 (include/sir_hip.h); the rows around them keep the bits of the all-good call."""
    fz = get_featurizer()
    lens = cases.lengths_for(SR16)
    x = cases.clips(SR16)
    rng = np.random.default_rng(21)
    cents = rng.uniform(-200.0, 200.0, len(lens)).astype(np.float32)
    tempo = rng.uniform(0.5, 2.0, len(lens)).astype(np.float32)
    M = _full_len(SR16)
    base_out, base_len, base_offs = _call(fz, x, lens, M, cents=cents, tempo=tempo)
    assert int(base_len[0]) > 0 and int(base_len[10]) > 0
    bad_cents, bad_tempo = cents.copy(), tempo.copy()
    bad_cents[0] = np.nextafter(_f32(200), _f32(300))
    bad_tempo[10] = np.nextafter(_f32(2), _f32(3))
    offs = torch.full((len(lens), 2, cases.max_segments(SR16)), 7, dtype=torch.int32, device="cuda")
    out, out_len = fz.perturb(x.cuda(), _dev(lens, torch.int32), pitch_cents=_dev(bad_cents, torch.float32),
                              tempo=_dev(bad_tempo, torch.float32), max_out_len=M, offsets_out=offs)
    with pytest.raises(_native.SirError):
        ops.check_status()
    ops.check_status()
    out, out_len, offs = out.cpu(), out_len.cpu(), offs.cpu().numpy()
    for b in (0, 10):
        assert int(out_len[b]) == 0 and (out[b] == 0).all() and (offs[b, 1] == -1).all(), b
    assert (offs[0, 0] == -1).all() and np.array_equal(offs[10, 0], base_offs[10, 0])
    assert torch.equal(out[1:10].view(torch.int32), base_out[1:10].view(torch.int32))
    assert torch.equal(out_len[1:10], base_len[1:10]) and np.array_equal(offs[1:10], base_offs[1:10])


def test_lengths_are_clamped_to_the_batch():
    fz = get_featurizer()
    lens = cases.lengths_for(SR16)
    x = cases.clips(SR16)
    x[0] = cases.clips(SR16, seed=5)[0]                                  # full rows, so that a clamped length reads real samples
    x[2] = cases.clips(SR16, seed=6)[0]
    rng = np.random.default_rng(9)
    cents = rng.uniform(-200.0, 200.0, len(lens)).astype(np.float32)
    tempo = rng.uniform(0.5, 2.0, len(lens)).astype(np.float32)
    wild, clamped = list(lens), list(lens)
    wild[0], clamped[0] = 2 * SR16 + 1, 2 * SR16
    wild[2], clamped[2] = 2 ** 31 - 1, 2 * SR16
    wild[3], clamped[3] = -1, 0
    wild[5], clamped[5] = -2 ** 31, 0
    for kw in ({"tempo": tempo}, {"cents": cents}, {"cents": cents, "tempo": tempo}):
        M = _full_len(SR16) if "tempo" in kw else 2 * SR16
        a = _call(fz, x, wild, M, **kw)
        b = _call(fz, x, clamped, M, **kw)
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
        assert np.array_equal(a[2], b[2])
        assert int(a[1][3]) == 0 and int(a[1][5]) == 0 and int(a[1][0]) > 0


@pytest.mark.parametrize("sr", [7999, 24001])
def test_rate_outside_the_lds_window_is_refused_by_the_call(sr):
    fz = HipFeaturizer(sr)                                               # sir_create_ex takes any positive sample rate
    x = cases.clips(SR16)[:2, :4000].contiguous()
    for kw in ({"tempo": np.float32([0.9, 1.1])}, {"cents": np.float32([50.0, -50.0])}):
        rc, out, out_len, offs = _raw(fz, x, [4000, 3000], 4800, 4800, check=False, **kw)
        assert rc == _native.SIR_EUNSUPPORTED
        assert (out == SENTINEL).all() and (out_len == -7).all() and (offs == 7).all()
        assert str(sr).encode() in _native.lib().sir_last_error()
    _status(fz)
    with pytest.raises(_native.SirError):
        fz.perturb(x.cuda(), tempo=torch.tensor([0.9, 1.1]))


def test_features_of_range_end_tempo_rows_match_oracle():
    """tests/test_wave_perturb_gpu.py::test_perturbed_features_match_oracle at the ends of the tempo range."""
    fz = get_featurizer()
    lens = [40000, 48000, 30000, 30000, 5000, 1312, 300, 47999]
    x = synth.synth_clips(len(lens), 48000, seed=31)
    for b, n in enumerate(lens):
        x[b, n:] = 0
    tempo = torch.tensor([0.5, 2.0] * 4)
    M = cases.round_up4(2 * 40000 + 4)
    assert all(ref.out_len(n, float(f)) <= M for n, f in zip(lens, tempo))
    offs = torch.full((len(lens), 2, 96), 7, dtype=torch.int32, device="cuda")
    wave, wlen = fz.perturb(x.cuda(), torch.tensor(lens, dtype=torch.int32, device="cuda"), tempo=tempo.cuda(), max_out_len=M,
                            offsets_out=offs)
    feats = fz(wave, wlen, t_pad=200).cpu()
    ops.check_status()
    offs, wlen = offs.cpu().numpy(), wlen.cpu()
    for b, n in enumerate(lens):
        z = ref.tempo(x[b, :n].double().numpy(), float(tempo[b]), offsets=offs[b, 1])[0]
        assert len(z) == int(wlen[b]) == ref.out_len(n, float(tempo[b]))
        f = features_ref.extract_features_f32(torch.from_numpy(z).float())
        if f is None:                                                    # <= 512 samples: the reference's zero spectrogram
            assert (feats[b] == 0).all(), b
            continue
        want = features_ref.pad_or_trim(f)
        err = ((feats[b] - want).abs() / want.abs().clamp(min=1.0)).max().item()
        assert err <= 1e-4, (b, err)
