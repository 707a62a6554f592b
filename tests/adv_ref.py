"""Host restatement of ``sir_adv_step`` (csrc/adversarial.hip) in numpy float32, and of ``train_ops.Adversary``'s host draws.

Every arithmetic step is one float32 numpy operation, i.e. one rounding, as the kernel's ``__fadd_rn`` / ``__fsub_rn`` /
``__fmul_rn`` are; kept elements are selected as 32-bit words, never computed.  ``fmaxf`` / ``fminf`` are restated with the
semantics of the gfx950 ``v_max_f32`` / ``v_min_f32`` instructions they compile to: a NaN operand yields the other operand, and
-0.0 orders below +0.0 (numpy's ``fmax`` / ``fmin`` return their first argument for the two zeros, which is order-dependent).

The self-check (``check_uniform_against_dropout_keep``) pins the integer part of the uniform to ``host_rng.dropout_keep``: the
keep mask of that function is ``U >= p``, so the two must agree for every threshold ``p``.
"""
import random

import numpy as np

import host_rng

F32 = np.float32


def uniform24(seed, n):
    """float32 [n]: the 24-bit uniform of element indices 0..n-1 (hash of (seed, idx), ``>> 40``, ``* 2^-24``)."""
    with np.errstate(over="ignore"):
        idx = np.arange(n, dtype=np.uint64)
        x = np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) ^ (idx * np.uint64(0x9E3779B97F4A7C15))
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xFF51AFD7ED558CCD)
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xC4CEB9FE1A85EC53)
        x ^= x >> np.uint64(33)
    return (x >> np.uint64(40)).astype(np.uint32).astype(F32) * F32(1.0 / 16777216.0)


def check_uniform_against_dropout_keep(seed, n, ps=(0.0, 0.1, 0.5, 0.9, 1.0)):
    u = uniform24(seed, n)
    assert u.dtype == F32 and (u >= 0).all() and (u < 1).all()
    for p in ps:
        assert np.array_equal(u >= F32(p), host_rng.dropout_keep(seed, n, p)), p
    return u


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def fmaxf(a, b):
    out = np.fmax(a, b)                                  # NaN handling: the other operand
    both_zero = (a == 0) & (b == 0)
    return np.where(both_zero, (_bits(a) & _bits(b)).view(F32), out)      # +0.0 unless both are -0.0


def fminf(a, b):
    out = np.fmin(a, b)
    both_zero = (a == 0) & (b == 0)
    return np.where(both_zero, (_bits(a) | _bits(b)).view(F32), out)      # -0.0 if either is


def zero_columns(x0):
    """bool [B, 1, T]: frame columns whose n_mels values are all bit pattern 0 (+0.0; a -0.0 is data)."""
    return (_bits(x0) == 0).all(axis=1, keepdims=True)


def sign_step(g, alpha):
    """``s * alpha`` as the kernel forms it: a select among ``alpha``, ``-alpha`` and ``+0.0`` (NaN compares false twice)."""
    g = np.asarray(g)
    alpha = F32(alpha)
    return np.where(g > 0, alpha, np.where(g < 0, -alpha, F32(0.0))).astype(F32)


def adv_step(x0, x=None, g=None, eps=0.0, alpha=0.0, active=None, seed=0, keep_zero_columns=True, step=None):
    """float32 [B, n_mels, T]: what ``sir_adv_step`` writes.  ``g`` (or a ready ``step = sign_step(g, alpha)``) given: the
    gradient step from ``x``; neither: the random start keyed by ``seed``."""
    x0 = np.ascontiguousarray(x0, dtype=F32)
    bsz, n_mels, t = x0.shape
    eps = F32(eps)
    with np.errstate(invalid="ignore", over="ignore"):
        if g is not None or step is not None:
            if step is None:
                step = sign_step(g, alpha)
            y = np.asarray(x, dtype=F32) + step
        else:
            assert x is None
            u = uniform24(seed, x0.size).reshape(x0.shape)
            r = F32(2.0) * u - F32(1.0)
            y = x0 + eps * r
        lo, hi = x0 - eps, x0 + eps
        moved = fminf(fmaxf(y.astype(F32), lo), hi).astype(F32)
    keep = np.zeros(x0.shape, dtype=bool)
    if active is not None:
        keep |= (np.asarray(active).reshape(bsz, 1, 1) == 0)
    if keep_zero_columns:
        cols = zero_columns(x0)
        if active is not None:
            cols = cols & (np.asarray(active).reshape(bsz, 1, 1) != 0)
        keep |= cols
    return np.where(keep, _bits(x0), _bits(moved)).view(F32)


def default_alpha(eps, steps, random_start):
    if steps == 1:
        return 1.25 * eps if random_start else eps
    return 2.5 * eps / steps


class AdversaryDraws:
    """``train_ops.Adversary``'s host stream restated: per batch ``bsz`` uniform draws (flag = draw < prob), then 64 bits."""

    def __init__(self, prob=1.0, seed=0):
        self.prob, self.rng = float(prob), random.Random(int(seed))

    def draw(self, bsz):
        flags = [1 if self.rng.random() < self.prob else 0 for _ in range(bsz)]
        return flags, self.rng.getrandbits(64)
