"""float64 numpy restatement of the cosine-proxy loss and its gradients (include/sir_hip.h: sir_proxy_loss), taking the fp32
inputs as given; the same loss in torch float64 for autograd; an fp32 restatement of the kernel's arithmetic in numpy; and the
bounds the tests hold the kernel to.

Every bound is derived, none is measured.  With eps = 2^-24 and proto_ref.SIM_BOUND = 600 eps per similarity (a 512-term fp32 dot
product of unit vectors in any order, the fp32 rounding of both unit vectors, the two roundings that form the logit):
  logit      |dz_logit| <= scale * SIM_BOUND
  row loss   log-sum-exp moves by at most the largest logit error and the label's logit by its own: 2 scale SIM_BOUND, plus expf,
             the float log argument and the final rounding: 8 eps (1 + |loss|)
  softmax    proto_ref.prob_bound(p, scale)
  dz         |gs| (prob_bound(p) + 2 eps) with gs = grad_scale / n_valid (the subtraction of the onehot and the product)
  du, dq     a sum of n = P (or B) terms dz * unit: scale * (sum of the dz bounds times |unit| + (n + 10) eps sum |dz| |unit|), the
             second term being the fp32 accumulation in any order, the rounding of the unit vector and the product with scale
  projection d - <d, v> v in double with the fp32 v: the bound of d, plus |v| times the bound of <d, v> (sum of bound_j |v_j|, and
             2 eps sum |d_j v_j| for the rounded v), all over the norm, plus the final rounding eps |result|
The fp32 restatement below measures how much of that room the arithmetic uses (tests/test_proxy_loss_host.py prints it)."""
import numpy as np

import proto_ref

DIM = 512
EPS = 2.0 ** -24
IGNORE = -100


def unit(rows):
    r = np.asarray(rows, dtype=np.float32).astype(np.float64)
    norm = np.sqrt((r * r).sum(axis=1))
    return r / norm[:, None], norm


def project(d, v, norm):
    return (d - (d * v).sum(axis=1, keepdims=True) * v) / norm[:, None]


def loss_and_grads(emb, proxies, labels, scale, margin, grad_scale=1.0):
    """float64 -> dict: loss, row_loss [B] (0 for ignored rows), z, prob, dz [B, P], du, dq, demb [B, 512], dproxies [P, 512], u, q,
    enorm, pnorm, n_valid, gs.  A label outside [0, P) that is not -100: loss NaN (the rows' gradients are not defined here)."""
    labels = np.asarray(labels, dtype=np.int64)
    u, enorm = unit(emb)
    q, pnorm = unit(proxies)
    n, p = u.shape[0], q.shape[0]
    valid = labels != IGNORE
    n_valid = int(valid.sum())
    y = np.where(valid, labels, 0)
    bad = valid & ((labels < 0) | (labels >= p))
    y = np.where(bad, 0, y)
    onehot = np.zeros((n, p))
    onehot[np.arange(n), y] = 1.0
    z = scale * (u @ q.T - margin * onehot)
    zs = z - z.max(axis=1, keepdims=True)
    e = np.exp(zs)
    den = e.sum(axis=1, keepdims=True)
    prob = e / den
    row_loss = np.where(valid, np.log(den[:, 0]) - zs[np.arange(n), y], 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        gs = np.float64(grad_scale) / np.float64(n_valid)
        loss = row_loss.sum() / np.float64(n_valid)
        dz = np.where(valid[:, None], (prob - onehot) * gs, 0.0)
    if bad.any():
        loss = np.nan
    du = scale * (dz @ q)
    live = np.where(valid[:, None], u, 0.0)                    # (an ignored row's embedding takes no part, whatever it holds)
    dq = scale * (dz.T @ live)
    demb = np.where(valid[:, None], project(du, u, enorm), 0.0)
    return {"loss": loss, "row_loss": row_loss, "z": z, "prob": prob, "dz": dz, "du": du, "dq": dq, "demb": demb,
            "dproxies": project(dq, q, pnorm), "u": u, "q": q, "enorm": enorm, "pnorm": pnorm, "n_valid": n_valid, "gs": gs,
            "valid": valid}


def loss_torch(emb, proxies, labels, scale, margin):
    """The same loss on torch tensors (any float dtype; the tests pass float64), differentiable by autograd."""
    import torch
    u = emb / emb.norm(dim=1, keepdim=True)
    q = proxies / proxies.norm(dim=1, keepdim=True)
    valid = labels != IGNORE
    y = torch.where(valid, labels, torch.zeros_like(labels))
    z = scale * (u @ q.T - margin * torch.nn.functional.one_hot(y, q.shape[0]).to(u.dtype))
    row = torch.logsumexp(z, dim=1) - z.gather(1, y[:, None])[:, 0]
    return (row * valid.to(u.dtype)).sum() / valid.sum()


# ---- bounds -----------------------------------------------------------------------------------------------------------------
def loss_bound(ref, scale):
    return 2.0 * scale * proto_ref.SIM_BOUND + 8.0 * EPS * (1.0 + abs(float(ref["loss"])))


def dz_bound(ref, scale):
    """[B, P]; zero on ignored rows (the kernel writes exact zeros there)"""
    b = abs(float(ref["gs"])) * (proto_ref.prob_bound(ref["prob"], scale) + 2.0 * EPS)
    return np.where(ref["valid"][:, None], b, 0.0)


def _projected_bound(d, d_bound, v, norm, result):
    av = np.abs(v)
    t_bound = (d_bound * av).sum(axis=1, keepdims=True) + 2.0 * EPS * (np.abs(d) * av).sum(axis=1, keepdims=True)
    return (d_bound + av * t_bound) / norm[:, None] + EPS * np.abs(result)


def demb_bound(ref, scale):
    n_terms = ref["q"].shape[0]
    aq = np.abs(ref["q"])
    du_b = scale * (dz_bound(ref, scale) @ aq + (n_terms + 10) * EPS * (np.abs(ref["dz"]) @ aq))
    return np.where(ref["valid"][:, None], _projected_bound(ref["du"], du_b, ref["u"], ref["enorm"], ref["demb"]), 0.0)


def dproxies_bound(ref, scale):
    n_terms = ref["u"].shape[0]
    au = np.where(ref["valid"][:, None], np.abs(ref["u"]), 0.0)
    dq_b = scale * (dz_bound(ref, scale).T @ au + (n_terms + 10) * EPS * (np.abs(ref["dz"]).T @ au))
    return _projected_bound(ref["dq"], dq_b, ref["q"], ref["pnorm"], ref["dproxies"])


# ---- the kernel's arithmetic in numpy float32 -------------------------------------------------------------------------------
def restate_f32(emb, proxies, labels, scale, margin, grad_scale=1.0):
    """fp32 unit vectors, proto_ref.sims_f32's dot product, fp32 logits and expf, the denominator and the quotient in double, fp32
    dz; du / dq by numpy's own fp32 matrix product (a different but fixed summation order), the projections in double on the fp32
    unit vectors, results rounded to fp32.  All rows must carry a label in range or -100."""
    labels = np.asarray(labels, dtype=np.int64)
    f32 = np.float32
    u64, enorm = unit(emb)
    q64, pnorm = unit(proxies)
    u32, q32 = u64.astype(f32), q64.astype(f32)
    n, p = u32.shape[0], q32.shape[0]
    valid = labels != IGNORE
    y = np.where(valid, labels, 0)
    onehot = np.zeros((n, p), f32)
    onehot[np.arange(n), y] = 1.0
    sims = proto_ref.sims_f32(np.asarray(emb, f32), q32)
    z = f32(scale) * (sims - f32(margin) * onehot)
    mx = z.max(axis=1, keepdims=True)
    e = np.exp((z - mx).astype(f32)).astype(f32)
    den = e.astype(np.float64).sum(axis=1, keepdims=True)
    row = (np.log(den[:, 0]) - (z[np.arange(n), y] - mx[:, 0]).astype(np.float64)).astype(f32)
    n_valid = int(valid.sum())
    loss = f32(np.where(valid, row, f32(0)).astype(np.float64).sum() / n_valid)
    gs = f32(grad_scale) / f32(n_valid)
    dz = np.where(valid[:, None], ((e.astype(np.float64) / den).astype(f32) - onehot) * gs, f32(0)).astype(f32)
    du = (f32(scale) * (dz @ q32)).astype(f32)
    dq = (f32(scale) * (dz.T @ np.where(valid[:, None], u32, f32(0)))).astype(f32)
    demb = project(du.astype(np.float64), u32.astype(np.float64), enorm).astype(f32)
    dprox = project(dq.astype(np.float64), q32.astype(np.float64), pnorm).astype(f32)
    return {"loss": loss, "dz": dz, "demb": np.where(valid[:, None], demb, f32(0)), "dproxies": dprox}


def make_case(batch, n_proxies, seed, ignore=()):
    """emb [B, 512], proxies [P, 512] (not unit), labels int64 [B] for a shape, deterministic"""
    rng = np.random.default_rng(seed)
    emb = rng.standard_normal((batch, DIM)).astype(np.float32) * np.float32(0.7)
    proxies = (rng.standard_normal((n_proxies, DIM)) * rng.uniform(0.25, 4.0, (n_proxies, 1))).astype(np.float32)
    labels = rng.integers(0, n_proxies, batch).astype(np.int64)
    # pull each row towards its proxy so that the softmax is neither flat nor saturated
    emb = (emb + np.float32(0.08) * proxies[labels] / np.linalg.norm(proxies[labels], axis=1, keepdims=True).astype(np.float32) *
           np.float32(np.sqrt(DIM) * 0.7)).astype(np.float32)
    for b in ignore:
        labels[b] = IGNORE
    return emb, proxies, labels


# ---- the joint loss through the model, float64 under autograd ---------------------------------------------------------------
def joint_reference(sd, x, labels, proxies, scale, margin, zo, yo, frames=None, ce_weight=1.0, proxy_weight=1.0):
    """ce_weight * CE(logits) + proxy_weight * loss_torch(ctx) in float64 at the device's forward values (z / y overrides):
    -> (loss, {parameter: gradient}, dx [B, 64, T], dproxies).  ``frames`` None: one padded batch with live batch statistics
    (``model_ref.forward(train=True)``); else clip by clip on the running statistics, as tests/ragged_grad_ref.py states the ragged
    function.  ``ctx`` comes from ``model_ref.forward(..., stages=...)``."""
    import torch
    import torch.nn.functional as F
    from oracle import model_ref
    d = lambda v: v.double() if torch.is_tensor(v) and v.is_floating_point() else v
    params = {k: sd[k].detach().double().clone().requires_grad_(True) for k in model_ref.PARAM_KEYS}
    full = {k: d(v) for k, v in sd.items()}
    full.update(params)
    bsz, t = x.shape[0], x.shape[-1]
    p64 = torch.as_tensor(proxies).detach().cpu().double().clone().requires_grad_(True)
    if frames is None:
        xs = [x.detach().cpu().double().view(bsz, 64, t).clone().requires_grad_(True)]
        st = {}
        logits = model_ref.forward(full, xs[0], train=True, new_stats={}, stages=st, z_override={k: d(v) for k, v in zo.items()},
                                   y_override={k: d(v) for k, v in yo.items()})
        ctx = st["ctx"]
    else:
        xs, rows, ctxs = [], [], []
        for b, f in enumerate(frames):
            xb = x[b].detach().cpu().double().view(64, t)[None, :, :f].clone().requires_grad_(True)
            xs.append(xb)
            w = {1: f, 2: f // 2, 3: f // 4}
            st = {}
            rows.append(model_ref.forward(full, xb, train=False, stages=st, z_override={i: d(zo[i][b:b + 1, :, :, :w[i]]) for i in w},
                                          y_override={i: d(yo[i][b:b + 1, :, :, :w[i]]) for i in w}))
            ctxs.append(st["ctx"])
        logits, ctx = torch.cat(rows, 0), torch.cat(ctxs, 0)
    loss = ce_weight * F.cross_entropy(logits, labels) + proxy_weight * loss_torch(ctx, p64, labels, scale, margin)
    grads = torch.autograd.grad(loss, [params[k] for k in model_ref.PARAM_KEYS] + xs + [p64], allow_unused=True)
    n = len(model_ref.PARAM_KEYS)
    pg = {k: (g if g is not None else torch.zeros_like(params[k])) for k, g in zip(model_ref.PARAM_KEYS, grads[:n])}
    dx = torch.zeros(bsz, 64, t, dtype=torch.float64)
    if frames is None:
        dx = grads[n]
    else:
        for b, (f, g) in enumerate(zip(frames, grads[n:-1])):
            dx[b, :, :f] = g[0]
    return loss.detach(), pg, dx, grads[-1]
