"""float64 statement of the three pieces of the training recipe (soft-target cross-entropy, batch mixing, gradient-norm
clipping), written from their definitions -- not through ``F.cross_entropy`` or ``clip_grad_norm_``, against which
tests/test_recipe_host.py checks them.  tests/test_recipe_gpu.py compares the HIP kernels with these."""
import torch

IGNORE = -100


def soft_targets(ya, yb, lam, eps, num_classes):
    """q[b] = (1 - eps) (lam[b] e[ya[b]] + (1 - lam[b]) e[yb[b]]) + eps / C, float64 [B, C]; ignored rows (ya == -100) are zero."""
    bsz = ya.numel()
    yb = ya if yb is None else yb
    lam = torch.ones(bsz, dtype=torch.float64) if lam is None else lam.double()
    q = torch.zeros(bsz, num_classes, dtype=torch.float64)
    for b in range(bsz):
        if int(ya[b]) == IGNORE:
            continue
        q[b, int(ya[b])] += (1.0 - eps) * float(lam[b])
        q[b, int(yb[b])] += (1.0 - eps) * (1.0 - float(lam[b]))
        q[b] += eps / num_classes
    return q


def soft_ce(logits, ya, yb=None, lam=None, eps=0.0):
    """(loss, dlogits) of the mean soft-target cross-entropy over the rows with ya != -100, in float64."""
    lg = logits.double()
    q = soft_targets(ya, yb, lam, eps, lg.shape[1])
    valid = (ya != IGNORE).double()[:, None]
    n_valid = valid.sum()
    z = lg - lg.max(dim=1, keepdim=True).values
    logp = z - z.exp().sum(dim=1, keepdim=True).log()
    loss = -(q * logp).sum() / n_valid
    dlogits = (logp.exp() * valid - q) / n_valid
    return loss, dlogits


def loss_case(bsz, ncls, second, seed):
    """The seeded case of the loss comparisons (tests/test_recipe_gpu.py, tests/test_class_count_gpu.py): logits 3 * randn,
    labels, with ``second`` a second label and a weight per row (0 in row 0, 1 in row 1, both labels on one class in row 3); rows
    2 and B - 1 are ignored, and the second label of an ignored row is invalid because it is not read."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(bsz, ncls, generator=g) * 3.0
    ya = torch.randint(0, ncls, (bsz,), generator=g)
    yb = lam = None
    if second:
        yb = torch.randint(0, ncls, (bsz,), generator=g)
        lam = torch.rand(bsz, generator=g)
        lam[0], lam[1] = 0.0, 1.0
        yb[3] = ya[3]                                  # both labels on one class
    ya[2] = IGNORE                                     # ignored rows (their second label is not read: make it invalid)
    ya[bsz - 1] = IGNORE
    if second:
        yb[2] = 10 ** 6
    return logits, ya, yb, lam


def mix(x, perm, lam, complement=None):
    """lam[b] x[b] + (1 - lam[b]) x[perm[b]] in float64.  ``complement`` (one value per row) replaces the real-number
    1 - lam[b], e.g. by the fp32 difference ``1.0f - lam`` the kernel forms."""
    xd = x.double()
    shape = (-1,) + (1,) * (x.dim() - 1)
    l = lam.double().view(shape)
    om = (1.0 - l) if complement is None else complement.double().view(shape)
    return l * xd + om * xd[perm]


def clip(grads, max_norm):
    """(total_norm, coef, scaled gradients) of clip_grad_norm_'s definition in float64:
    coef = min(1, max_norm / (total_norm + 1e-6))."""
    total = torch.sqrt(sum((g.double() ** 2).sum() for g in grads))
    coef = torch.clamp(max_norm / (total + 1e-6), max=1.0)
    return total, coef, [g.double() * coef for g in grads]
