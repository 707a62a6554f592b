"""GPU: sir_wave_reverb_mix against the float64 oracle at the sizes it runs at: every ring size with the ring wrapping more than
twice (tests/reverb_cases.py; test_reverb_scale_host.py shows that those cases tell a correct ring from a broken one), the
workload's clip lengths, the noise stage at clip length, and the row, batch, layout and extreme-SNR lines of include/sir_hip.h.

Bounds are the stage's own (test_reverb_gpu.py): max |out - oracle| <= 1e-5 |x|_inf |h|_1 per reverberated row, gain within 1e-5
relative, noise within 1e-5 (|y|_inf + g |v|_inf).  Every figure is printed (pytest -s) ahead of its assertion."""
import functools

import numpy as np
import pytest
import torch

import reverb_cases as rc
import reverb_ref as ref
from reverb_call import NAN, bank, call
from sir_amd import _native, ops, synth

pytestmark = pytest.mark.gpu

BOUND = 1e-5
INT_MIN, INT_MAX = -2147483648, 2147483647


@pytest.fixture(scope="module")
def fz():
    from sir_amd.featurizer import get_featurizer
    return get_featurizer()


def _padded(x, lengths, stride, fill):
    """[B][stride] on the GPU: row b holds x[b, :lengths[b]] and `fill` behind it"""
    w = torch.full((len(lengths), stride), fill, dtype=x.dtype)
    for b, n in enumerate(lengths):
        w[b, :n] = x[b, :n]
    return w.cuda()


def _f64(x):
    return x.double().numpy() / (32768.0 if x.dtype == torch.int16 else 1.0)


def _check_frame(out, lengths, max_len):
    o = out.cpu()
    for b, n in enumerate(lengths):
        assert torch.isfinite(o[b, :max_len]).all(), b
        assert (o[b, n:max_len] == 0).all(), b
        assert torch.isnan(o[b, max_len:]).all(), b               # columns >= max_len untouched


# ---- the spectrum ring at every size ---------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _ring_out(fz, case):
    """the kernel's output for one case of the table, as a CPU tensor; run once per case"""
    c = rc.ring_case(*case)
    lengths, index = [n for _, _, n in c["rows"]], [r for _, r, _ in c["rows"]]
    w = _padded(c["wave"], lengths, c["max_len"] + 8, 30000 if case[1] else NAN)
    rcode, out, gain = call(fz, w, lengths, rir=bank(c["rirs"], NAN), rir_index=index, max_len=c["max_len"],
                            max_rir_len=c["max_rir_len"], out_stride=c["max_len"] + 16)
    assert rcode == 0
    ops.check_status()
    assert not gain.any()
    _check_frame(out, lengths, c["max_len"])
    return out.cpu()


@pytest.mark.parametrize("case", rc.CASES, ids=rc.case_id)
def test_ring_wraps_at_every_size(fz, case):
    c, want, out = rc.ring_case(*case), rc.oracle(*case), _ring_out(fz, case)
    worst = 0.0
    for b, (_, r, n) in enumerate(c["rows"]):
        if r < 0:
            deq = c["wave"][b].float() / 32768.0 if case[1] else c["wave"][b]
            assert torch.equal(out[b, :n], deq[:n])               # index -1: the input bit for bit
            continue
        y64, bound = want[b]
        ratio = np.abs(out[b, :n].double().numpy() - y64).max() / bound
        worst = max(worst, ratio)
        assert ratio <= BOUND, (b, c["names"][r], ratio)
    print(f"parts {c['parts']:2d} (max_rir_len {case[0]}{', PCM16' if case[1] else ''}): max |out - oracle| / (|x|_inf |h|_1) = {worst:.3e}")


def test_ring_size_does_not_change_a_rows_bits(fz):
    """row 7 of a call (P = parts - 1 in a ring sized for parts) is row 0 of the call one partition smaller: same taps, same
    waveform, same length, another LDS layout"""
    pairs = 0
    for m in rc.MAX_RIR_LENS:
        c = rc.ring_case(m)
        if len(c["rows"]) < 8:
            continue
        _, r, n = c["rows"][7]
        k = len(c["rirs"][r])
        small = rc.ring_case(k)
        assert small["rows"][0] == (0, 0, n) and np.array_equal(small["rirs"][0], c["rirs"][r]) and small["parts"] == c["parts"] - 1
        assert torch.equal(_ring_out(fz, (m, False))[7, :n], _ring_out(fz, (k, False))[0, :n]), (m, k)
        pairs += 1
    assert pairs == 17
    print(f"bit-equal across max_rir_len: {pairs} pairs of calls")


# ---- the workload's own lengths ----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _clip_data():
    gen = np.random.default_rng(2025)
    x = synth.synth_clips(4, 160000, seed=57)
    rirs = [synth.synthetic_rir(0.6, rng=gen).numpy(), synth.synthetic_rir(0.1, rng=gen).numpy()]      # K = 8192 and 1600
    noises = [synth.coloured_noise(20000, gen).numpy(), (0.2 * gen.standard_normal(700)).astype(np.float32)]
    assert [len(h) for h in rirs] == [8192, 1600]
    return x, synth.to_int16(x), rirs, noises


@pytest.mark.parametrize("pcm16", [False, True], ids=["f32", "pcm16"])
@pytest.mark.parametrize("max_len,lengths", [(48000, [48000, 47999, 30000, 47489]), (160000, [160000, 159745])],
                         ids=["48000", "160000"])
def test_clip_lengths_reverb_then_noise(fz, max_len, lengths, pcm16):
    """94 and 313 blocks: a 3 s clip and a max_utterance clip, K = 8192 and 1600 in turn, each followed by noise"""
    x32, x16, rirs, noises = _clip_data()
    x = (x16 if pcm16 else x32)[:len(lengths), :max_len]
    ridx, nidx = [0, 1, 0, 1][:len(lengths)], [0, 1, 1, 0][:len(lengths)]
    offs, snrs = [19999, 5, 699, 123][:len(lengths)], [10.0, 0.0, -5.0, 20.0][:len(lengths)]
    w = _padded(x, lengths, max_len + 8, 30000 if pcm16 else NAN)
    rcode, out, gain = call(fz, w, lengths, rir=bank(rirs, NAN), rir_index=ridx, noise=bank(noises, NAN), noise_index=nidx,
                            noise_offset=offs, snr_db=snrs, max_len=max_len, max_rir_len=8192, out_stride=max_len + 8)
    assert rcode == 0
    ops.check_status()
    _check_frame(out, lengths, max_len)
    x64 = _f64(x)
    want = ref.mix_batch(x64, lengths, rirs, ridx, noises, nidx, offs, snrs)
    worst = worst_g = 0.0
    for b, n in enumerate(lengths):
        o, y, g, used = want[b]
        bound = np.abs(x64[b, :n]).max() * np.abs(rirs[ridx[b]].astype(np.float64)).sum() + g * np.abs(used).max()
        worst = max(worst, np.abs(out[b, :n].cpu().double().numpy() - o).max() / bound)
        worst_g = max(worst_g, abs(gain[b] - g) / g)
    print(f"max_len {max_len} {'PCM16' if pcm16 else 'float32'}, reverb + noise: max error / bound = {worst:.3e}, "
          f"max relative gain error = {worst_g:.3e}")
    assert worst <= BOUND and worst_g <= BOUND


# ---- the noise stage at clip length ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _noise_data():
    gen = np.random.default_rng(404)
    return synth.synth_clips(6, 48000, seed=63), (0.1 * gen.standard_normal(48001)).astype(np.float32)


@pytest.mark.parametrize("m_of", [lambda n: 1, lambda n: 3, lambda n: 700, lambda n: n, lambda n: n + 1],
                         ids=["M1", "M3", "M700", "ML", "ML+1"])
@pytest.mark.parametrize("n", [48000, 47999])
def test_noise_at_clip_length(fz, n, m_of):
    """one row per offset, one call per SNR: up to 48000 wraps (M = 1), none (M = L + 1), offsets at both int32 ends"""
    x, v_all = _noise_data()
    m = m_of(n)
    v = v_all[:m] if m > 1 else np.array([0.07], dtype=np.float32)
    offs = [0, m - 1, -1, -m, INT_MIN, INT_MAX]
    lengths = [n] * len(offs)
    w = _padded(x, lengths, 48000, NAN)
    nbank = bank([v], NAN)
    x64 = _f64(x)
    worst_g = worst_o = 0.0
    for snr in (-5.0, 0.0, 20.0, 60.0):
        rcode, out, gain = call(fz, w, lengths, noise=nbank, noise_index=[0] * len(offs), noise_offset=offs, snr_db=[snr] * len(offs),
                                max_len=48000, out_stride=48008)
        assert rcode == 0
        ops.check_status()
        _check_frame(out, lengths, 48000)
        o_cpu = out.cpu().double().numpy()
        for b, off in enumerate(offs):
            o, y, g, used = ref.mix_row(x64[b, :n], None, v, off, snr)
            assert np.array_equal(used, v.astype(np.float64)[(off % m + np.arange(n)) % m])          # the mathematical residue
            worst_g = max(worst_g, abs(gain[b] - g) / g)
            worst_o = max(worst_o, np.abs(o_cpu[b, :n] - o).max() / (np.abs(y).max() + g * np.abs(used).max()))
    print(f"noise at L = {n}, M = {m}: max relative gain error = {worst_g:.3e}, max |out - oracle| / (|y|_inf + g |v|_inf) = {worst_o:.3e}")
    assert worst_g <= BOUND and worst_o <= BOUND


# ---- rows, batches, layouts -----------------------------------------------------------------------------------------------

SMALL = 1500


@functools.lru_cache(maxsize=None)
def _small_data():
    gen = np.random.default_rng(808)
    x = synth.synth_clips(8, SMALL, seed=71)
    rirs = [np.array([1.0, -0.5, 0.25], dtype=np.float32), synth.synthetic_rir(700.5 / 16000.0, rng=gen).numpy()]
    noises = [(0.1 * gen.standard_normal(5)).astype(np.float32), (0.1 * gen.standard_normal(333)).astype(np.float32)]
    return x, synth.to_int16(x), rirs, noises


def _small_kw(rows, rirs, noises, **layout):
    return dict(rir=bank(rirs, NAN, **layout), rir_index=[b % 2 for b in range(rows)], noise=bank(noises, NAN, **layout),
                noise_index=[(b // 2) % 2 for b in range(rows)], noise_offset=[3 * b - 4 for b in range(rows)], max_len=SMALL)


def test_lengths_outside_the_row_and_null(fz):
    x, _, rirs, noises = _small_data()
    w = x[:6].contiguous().cuda()
    kw = _small_kw(6, rirs, noises)
    snr = [6.0] * 6
    rcode, want, gwant = call(fz, w, [0, 0, SMALL, SMALL, SMALL, 700], snr_db=snr, out_stride=SMALL + 8, **kw)
    assert rcode == 0
    rcode, out, gain = call(fz, w, [-1, INT_MIN, SMALL + 1, INT_MAX, SMALL, 700], snr_db=snr, out_stride=SMALL + 8, **kw)
    assert rcode == 0
    ops.check_status()                                            # a length outside [0, max_len] is clamped, not a bad row
    assert not out[:2, :SMALL].any() and gain[0] == 0.0 and gain[1] == 0.0
    assert torch.equal(out[:, :SMALL], want[:, :SMALL]) and np.array_equal(gain, gwant)
    assert gain[2:].all() and torch.isnan(out[:, SMALL:]).all()
    rcode, full, gfull = call(fz, w, [SMALL] * 6, snr_db=snr, out_stride=SMALL + 8, **kw)
    rcode2, null, gnull = call(fz, w, None, snr_db=snr, out_stride=SMALL + 8, **kw)
    assert rcode == 0 and rcode2 == 0
    ops.check_status()
    assert torch.equal(null[:, :SMALL], full[:, :SMALL]) and np.array_equal(gnull, gfull) and torch.isnan(null[:, SMALL:]).all()
    ratio = np.abs(full[3, :SMALL].cpu().double().numpy() - ref.mix_row(_f64(x)[3], rirs[1], noises[1], 5, 6.0)[0]).max()
    assert ratio <= BOUND * (np.abs(_f64(x)[3]).max() * np.abs(rirs[1]).sum() + gfull[3] * np.abs(noises[1]).max())


def test_batch_of_one_with_dense_output(fz):
    x, _, rirs, noises = _small_data()
    buf = torch.full((SMALL + 8,), NAN, device="cuda")
    rcode, out, gain = call(fz, x[:1].contiguous().cuda(), [SMALL - 3], rir=bank(rirs, NAN), rir_index=[1], noise=bank(noises, NAN),
                            noise_index=[1], noise_offset=[-7], snr_db=[3.0], max_len=SMALL, out=buf[:SMALL].view(1, SMALL))
    assert rcode == 0 and out.stride(0) == SMALL
    ops.check_status()
    o, y, g, used = ref.mix_row(_f64(x)[0, :SMALL - 3], rirs[1], noises[1], -7, 3.0)
    bound = np.abs(_f64(x)[0]).max() * np.abs(rirs[1]).sum() + g * np.abs(used).max()
    assert np.abs(buf[:SMALL - 3].cpu().double().numpy() - o).max() <= BOUND * bound and abs(gain[0] - g) <= BOUND * g
    assert not buf[SMALL - 3:SMALL].any() and torch.isnan(buf[SMALL:]).all()


@functools.lru_cache(maxsize=None)
def _tiny_rows():
    """eight rows of eight PCM16 samples with noise only: the rows of the large batches, b -> row b % 8"""
    gen = np.random.default_rng(909)
    x = synth.to_int16(torch.from_numpy(gen.uniform(-0.9, 0.9, (8, 8)).astype(np.float32)))
    noises = [(0.1 * gen.standard_normal(3)).astype(np.float32), (0.1 * gen.standard_normal(11)).astype(np.float32)]
    return x, noises, dict(noise_index=[0, 1, -1, 1, 0, 0, 1, 1], noise_offset=[0, 10, 0, -1, INT_MIN, 2, INT_MAX, -11],
                           snr_db=[0.0, 20.0, 0.0, -5.0, 3.0, 60.0, 10.0, 0.0])


@pytest.mark.parametrize("batch", [300, 65535])
def test_more_rows_than_compute_units(fz, batch):
    """256 CUs; 65535 is the largest grid the entry point takes.  lengths = NULL keeps the call's input under 2 MB."""
    x, noises, kw = _tiny_rows()
    nbank = bank(noises, NAN)
    rcode, base, gbase = call(fz, x.cuda(), None, noise=nbank, max_len=8, out_stride=8, **kw)
    assert rcode == 0
    want = ref.mix_batch(_f64(x), [8] * 8, None, None, noises, kw["noise_index"], kw["noise_offset"], kw["snr_db"])
    for b in range(8):
        o, y, g, used = want[b]
        assert np.abs(base[b].cpu().double().numpy() - o).max() <= BOUND * (np.abs(y).max() + g * (np.abs(used).max() if g else 0.0)), b
    rep = -(-batch // 8)
    tile = lambda v: (v * rep)[:batch]
    rcode, out, gain = call(fz, x.repeat(rep, 1)[:batch].contiguous().cuda(), None, noise=nbank, max_len=8, out_stride=8,
                            noise_index=tile(kw["noise_index"]), noise_offset=tile(kw["noise_offset"]), snr_db=tile(kw["snr_db"]))
    assert rcode == 0
    ops.check_status()
    assert torch.equal(out, base.repeat(rep, 1)[:batch])
    assert np.array_equal(gain, np.tile(gbase, rep)[:batch])


def test_batch_beyond_the_grid_is_refused(fz):
    x, noises, kw = _tiny_rows()
    tile = lambda v: v * 8192
    sentinel = torch.full((65536, 8), 7.0, device="cuda")
    rcode, out, _ = call(fz, x.repeat(8192, 1).contiguous().cuda(), None, noise=bank(noises), max_len=8, out=sentinel,
                         noise_index=tile(kw["noise_index"]), noise_offset=tile(kw["noise_offset"]), snr_db=tile(kw["snr_db"]))
    assert rcode == _native.SIR_EINVAL and (out == 7.0).all()
    ops.check_status()


def test_odd_strides_wide_banks_and_the_last_bank_row(fz):
    _, x16, rirs, noises = _small_data()
    lengths = [SMALL, SMALL - 1, 1025, 513, 1, 700, 1499, 0]
    w = _padded(x16, lengths, SMALL + 1, 30000)                   # rows start on odd 2-byte offsets
    kw = _small_kw(8, rirs, noises, extra=20001)                  # bank strides of 20 k floats for 3 .. 700 of them
    assert w.stride(0) % 2 == 1 and kw["rir"][0].stride(0) > 20000 and kw["noise"][0].stride(0) > 20000
    kw["rir_index"][6] = kw["noise_index"][6] = 1                 # the last row of either bank
    snr = [0.0, 20.0, -5.0, 60.0, 0.0, 20.0, -5.0, 0.0]
    rcode, out, gain = call(fz, w, lengths, snr_db=snr, out_stride=SMALL + 3, **kw)
    assert rcode == 0 and out.stride(0) % 2 == 1
    ops.check_status()
    _check_frame(out, lengths, SMALL)
    x64 = _f64(x16)
    want = ref.mix_batch(x64, lengths, rirs, kw["rir_index"], noises, kw["noise_index"], kw["noise_offset"], snr)
    worst = worst_g = 0.0
    for b, n in enumerate(lengths):
        if n == 0:
            assert gain[b] == 0.0
            continue
        o, y, g, used = want[b]
        bound = np.abs(x64[b, :n]).max() * np.abs(rirs[kw["rir_index"][b]].astype(np.float64)).sum() + g * np.abs(used).max()
        worst = max(worst, np.abs(out[b, :n].cpu().double().numpy() - o).max() / bound)
        worst_g = max(worst_g, abs(gain[b] - g) / g)
    print(f"odd strides, wide banks, PCM16: max error / bound = {worst:.3e}, max relative gain error = {worst_g:.3e}")
    assert worst <= BOUND and worst_g <= BOUND


# ---- extreme finite SNR --------------------------------------------------------------------------------------------------

def test_extreme_finite_snr(fz):
    """a gain that is no finite float32 makes a bad row (zeroed, gain 0, status raised); a gain that underflows is no error"""
    x, _, rirs, noises = _small_data()
    lengths = [SMALL, 1400, SMALL, 1100, 1300, SMALL, 900, 1]
    w = _padded(x, lengths, SMALL + 8, NAN)
    kw = _small_kw(8, rirs, noises)
    clean_snr = [6.0] * 8
    rcode, clean, gclean = call(fz, w, lengths, snr_db=clean_snr, out_stride=SMALL + 8, **kw)
    assert rcode == 0
    dry = dict(kw, noise_index=[-1] * 8)
    rcode2, y, _ = call(fz, w, lengths, snr_db=clean_snr, out_stride=SMALL + 8, **dry)          # the reverb alone
    assert rcode2 == 0
    ops.check_status()
    x64 = _f64(x)
    oracle_row = lambda b, snr: ref.mix_row(x64[b, :lengths[b]], rirs[kw["rir_index"][b]], noises[kw["noise_index"][b]],
                                            kw["noise_offset"][b], snr)

    # 10^(snr / 10) overflows or is huge: the gain underflows to 0 or is tiny, the row is y
    snr = [3e38, 400.0, 3e38, 400.0] + clean_snr[4:]
    rcode, out, gain = call(fz, w, lengths, snr_db=snr, out_stride=SMALL + 8, **kw)
    assert rcode == 0
    ops.check_status()
    _check_frame(out, lengths, SMALL)
    for b in (0, 2):
        assert gain[b] == 0.0 and torch.equal(out[b, :SMALL], y[b, :SMALL]), b
    for b in (1, 3):
        o, yy, g, used = oracle_row(b, 400.0)
        assert 0.0 < g < 1e-15 and abs(gain[b] - g) <= BOUND * g, (b, g, gain[b])
        assert np.abs(out[b, :lengths[b]].cpu().double().numpy() - o).max() <= BOUND * (np.abs(yy).max() + g * np.abs(used).max()), b
    assert torch.equal(out[4:, :SMALL], clean[4:, :SMALL]) and np.array_equal(gain[4:], gclean[4:])

    # the gain overflows float32: a bad row
    for row, bad in ((0, -3e38), (3, -1000.0), (5, -3e38), (6, -1000.0)):
        assert not ref.noise_gain(oracle_row(row, 0.0)[1], oracle_row(row, 0.0)[3], bad)[1]
        snr = clean_snr[:row] + [bad] + clean_snr[row + 1:]
        rcode, out, gain = call(fz, w, lengths, snr_db=snr, out_stride=SMALL + 8, **kw)
        assert rcode == 0
        assert torch.isfinite(out[:, :SMALL]).all(), (row, bad)
        assert not out[row, :SMALL].any() and gain[row] == 0.0, (row, bad)
        others = [b for b in range(8) if b != row]
        assert torch.equal(out[others][:, :SMALL], clean[others][:, :SMALL]) and np.array_equal(gain[others], gclean[others]), (row, bad)
        assert torch.isnan(out[:, SMALL:]).all()
        with pytest.raises(_native.SirError, match="sir_wave_reverb_mix"):
            ops.check_status()
        ops.check_status()                                        # raised once: the word is cleared

    # large and finite: plain float32 arithmetic
    snr = clean_snr[:2] + [-300.0] + clean_snr[3:]
    rcode, out, gain = call(fz, w, lengths, snr_db=snr, out_stride=SMALL + 8, **kw)
    assert rcode == 0
    ops.check_status()
    o, yy, g, used = oracle_row(2, -300.0)
    assert 1e13 < g < 1e17 and abs(gain[2] - g) <= BOUND * g
    err = np.abs(out[2, :SMALL].cpu().double().numpy() - o).max() / (np.abs(yy).max() + g * np.abs(used).max())
    print(f"snr_db = -300: gain {gain[2]:.4e} (oracle {g:.4e}), max |out - oracle| / (|y|_inf + g |v|_inf) = {err:.3e}")
    assert err <= BOUND
    others = [b for b in range(8) if b != 2]
    assert torch.equal(out[others][:, :SMALL], clean[others][:, :SMALL])
