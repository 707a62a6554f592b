"""CPU: the float64 reference of the cosine-proxy loss against itself (tests/proxy_ref.py), the fp32 restatement of the kernel's
arithmetic inside the bounds the GPU test holds the kernel to, the ``metric_loss`` YAML key's refusals, and the ``ProxyHead`` <->
``PrototypeBank`` round trip where it needs no device."""
import numpy as np
import pytest
import torch

import proxy_ref


def _central_differences(fn, x, h):
    g = np.zeros_like(x)
    flat, gf = x.reshape(-1), g.reshape(-1)
    for i in range(flat.size):
        keep = flat[i]
        flat[i] = keep + h
        up = fn()
        flat[i] = keep - h
        down = fn()
        flat[i] = keep
        gf[i] = (up - down) / (2.0 * h)
    return g


@pytest.mark.parametrize("scale,margin", [(1.0, 0.0), (16.0, 0.2)])
def test_analytic_gradients_agree_with_finite_differences(scale, margin):
    """batch 5 x 7 proxies in float64, one row ignored, grad_scale 0.5: central differences of the loss with step 1e-6 carry a
    truncation error of h^2 f''' / 6 ~ 1e-10 and a rounding error of 2^-53 |loss| / h ~ 1e-9."""
    emb, proxies, labels = proxy_ref.make_case(5, 7, seed=1, ignore=(3,))
    ref = proxy_ref.loss_and_grads(emb, proxies, labels, scale, margin, grad_scale=0.5)
    e64, p64 = emb.astype(np.float64), proxies.astype(np.float64)

    def loss():
        # (the reference takes fp32 inputs as given; the differences need float64 inputs, so the same statements are evaluated
        # through the torch float64 form)
        return float(proxy_ref.loss_torch(torch.from_numpy(e64), torch.from_numpy(p64), torch.from_numpy(labels), scale, margin))

    assert abs(loss() - ref["loss"]) < 1e-12
    fe = 0.5 * _central_differences(loss, e64, 1e-6)
    fp = 0.5 * _central_differences(loss, p64, 1e-6)
    de, dp = np.abs(fe - ref["demb"]).max(), np.abs(fp - ref["dproxies"]).max()
    print(f"scale={scale} margin={margin}: analytic vs central differences: demb {de:.2e} (max {np.abs(ref['demb']).max():.2e}), "
          f"dproxies {dp:.2e} (max {np.abs(ref['dproxies']).max():.2e})")
    assert de < 2e-8 and dp < 2e-8
    assert np.all(ref["demb"][3] == 0.0) and np.abs(ref["demb"]).max() > 1e-4
    # autograd on the torch form agrees too (the joint-loss test differentiates it)
    et, pt = torch.from_numpy(e64).requires_grad_(), torch.from_numpy(p64).requires_grad_()
    proxy_ref.loss_torch(et, pt, torch.from_numpy(labels), scale, margin).backward()
    assert np.abs(0.5 * et.grad.numpy() - ref["demb"]).max() < 1e-14 and np.abs(0.5 * pt.grad.numpy() - ref["dproxies"]).max() < 1e-14


@pytest.mark.parametrize("bsz,n", [(5, 7), (17, 65), (17, 257), (65, 31)])
def test_fp32_restatement_stays_inside_the_bounds(bsz, n):
    """The kernel's arithmetic in numpy float32 against float64: how much of each derived bound it uses (printed)."""
    emb, proxies, labels = proxy_ref.make_case(bsz, n, seed=100 * bsz + n, ignore=(1,) if bsz > 1 else ())
    for scale in (1.0, 16.0, 64.0):
        for margin in (0.0, 0.2):
            ref = proxy_ref.loss_and_grads(emb, proxies, labels, scale, margin)
            got = proxy_ref.restate_f32(emb, proxies, labels, scale, margin)
            le = abs(float(got["loss"]) - ref["loss"]) / proxy_ref.loss_bound(ref, scale)
            valid = ref["valid"]
            ze = (np.abs(got["dz"] - ref["dz"])[valid] / proxy_ref.dz_bound(ref, scale)[valid]).max()
            ee = (np.abs(got["demb"] - ref["demb"])[valid] / proxy_ref.demb_bound(ref, scale)[valid]).max()
            pe = (np.abs(got["dproxies"] - ref["dproxies"]) / proxy_ref.dproxies_bound(ref, scale)).max()
            print(f"B={bsz} P={n} scale={scale} margin={margin}: error / bound: loss {le:.4f} dz {ze:.4f} demb {ee:.4f} dproxies {pe:.4f}")
            assert max(le, ze, ee, pe) <= 1.0
            assert np.all(got["demb"][~valid] == 0.0)


def test_metric_loss_key_refusals():
    from sir_amd.scripts import train as tr
    assert tr.metric_loss_options({}) is None
    got = tr.metric_loss_options({"metric_loss": {}})
    assert got == {"weight": 1.0, "ce_weight": 1.0, "scale": 16.0, "margin": 0.1, "bank_out": None}
    got = tr.metric_loss_options({"metric_loss": {"weight": 0.5, "ce_weight": 0, "scale": 30, "margin": 0, "bank_out": "p.npz"}})
    assert got == {"weight": 0.5, "ce_weight": 0.0, "scale": 30.0, "margin": 0.0, "bank_out": "p.npz"}
    for bad in ({"metric_loss": [1]}, {"metric_loss": {"wieght": 1}}, {"metric_loss": {"weight": -1}}, {"metric_loss": {"ce_weight": -1}},
                {"metric_loss": {"weight": 0, "ce_weight": 0}}, {"metric_loss": {"scale": 0}}, {"metric_loss": {"scale": float("inf")}},
                {"metric_loss": {"margin": -0.1}}, {"metric_loss": {"bank_out": ""}},
                {"metric_loss": {}, "mixup": 0.2}, {"metric_loss": {}, "adversarial": {"eps": 0.1}},
                {"metric_loss": {}, "slots": {"columns": ["action", "object"]}}):
        with pytest.raises(ValueError):
            tr.metric_loss_options(bad)


def test_proxy_head_bank_round_trip_on_the_host(tmp_path):
    from sir_amd.prototypes import PrototypeBank, ProxyHead
    names = ["lights on", "lights off", "volume up"]
    head = ProxyHead(3, names=names, scale=20.0, margin=0.2, seed=5)
    assert head.proxies.shape == (3, 512) and [n for n, _ in head.named_parameters()] == ["proxies"]
    assert torch.equal(head.proxies, ProxyHead(3, seed=5).proxies) and not torch.equal(head.proxies, ProxyHead(3, seed=6).proxies)
    with torch.no_grad():
        head.proxies[1] *= 7.0                           # the centres need not be unit
    bank = PrototypeBank.from_proxies(head)
    a = bank.state_arrays()
    unit = head.proxies.detach().double().numpy()
    unit /= np.sqrt((unit * unit).sum(axis=1, keepdims=True))
    assert bank.names == names and not bank.exemplars
    assert a["count"].tolist() == [1, 1, 1] and a["skipped"] == 0 and np.array_equal(a["sum"], unit)
    bank.save(tmp_path / "bank.npz")
    again = PrototypeBank.load(tmp_path / "bank.npz")
    assert again.names == names and np.array_equal(again.state_arrays()["sum"], unit)
    fresh = ProxyHead(3, names=names, seed=9).init_from_bank(again)
    assert torch.equal(fresh.proxies.detach(), torch.from_numpy(unit.astype(np.float32)))
    with pytest.raises(ValueError):
        ProxyHead(3, names=["a", "b", "c"]).init_from_bank(again)          # other names
    with pytest.raises(ValueError):
        ProxyHead(3, names=names).init_from_bank(PrototypeBank(names))      # nothing enrolled
    for bad in (dict(n_classes=0), dict(n_classes=4097), dict(n_classes=3, scale=0.0), dict(n_classes=3, margin=-1.0),
                dict(n_classes=3, names=["a", "a", "b"])):
        with pytest.raises(ValueError):
            ProxyHead(**bad)
