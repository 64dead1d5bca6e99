"""``ddr_amd.nn``: the reference's KAN (src/ddr/nn/kan.py:11-62) -- its state-dict contract against the weights
of both published checkpoints (tests/golden/kan_*.npz: weights, not reference results), the B-spline identities of
the layer's arithmetic, the reference's own test cases (tests/nn/test_kan.py) and the refusals.  CPU only:
``TorchKan`` in fp64, no HIP library needed.  Parity with pykan itself is not pinned (pykan cannot run here)."""

import numpy as np
import pytest
import torch

from conftest import load_golden
from ddr_amd.nn import TorchKan, kan

CKPT = dict(input_var_names=[f"a{i}" for i in range(10)], learnable_parameters=["n", "q_spatial", "p_spatial"],
            hidden_size=21, num_hidden_layers=2, grid=50, k=2, seed=0)


@pytest.mark.parametrize("name", ["kan_merit", "kan_lynker"])
@pytest.mark.parametrize("cls", [TorchKan, kan])
def test_strict_load_of_published_weights(name, cls):
    sd = {k: torch.from_numpy(v) for k, v in load_golden(name).items()}
    net = cls(**CKPT)
    net.load_state_dict(sd, strict=True)
    out = net.state_dict()
    assert list(out) == list(sd)  # the reference's keys, in its order
    for k, v in sd.items():
        assert out[k].shape == v.shape and out[k].dtype == v.dtype, k
        assert torch.equal(out[k], v), k
    assert net.flat.numel() == 47925 and list(dict(net.named_parameters())) == ["flat"]
    if cls is TorchKan:  # the published weights evaluate: outputs of N(0, 1) attributes in (0, 1)
        x = torch.randn(500, 10, generator=torch.Generator().manual_seed(1))
        with torch.no_grad():
            o = net.double()(inputs=x.double())
            h0 = x.double() @ net.views()["input.weight"].t() + net.views()["input.bias"]
        # with the trained weights a large share of the first layer's inputs lies outside the knots (|t| <= 1.08):
        # there only the SiLU branch is live -- the common case, not a corner
        assert float((h0.abs() > 1.08).double().mean()) > 0.25
        assert all(o[k].shape == (500,) and 0.0 < float(o[k].min()) and float(o[k].max()) < 1.0 for k in CKPT["learnable_parameters"])


def test_lazy_top_level_name():
    import ddr_amd

    assert ddr_amd.kan is kan


def _identity_net(H, G, k, uniform, seed):
    """F = H with the input Linear the identity; scale_base = 0, scale_sp = mask = 1: the layer is the bare spline sum."""
    net = TorchKan([f"a{i}" for i in range(H)], ["u"], H, 1, G, k, seed).double()
    v, c = net.views(), net.const_views()
    with torch.no_grad():
        v["input.weight"].copy_(torch.eye(H))
        v["input.bias"].zero_()
        v["layers.0.act_fun.0.scale_base"].zero_()
        v["layers.0.act_fun.0.scale_sp"].fill_(1.0)
        if not uniform:
            g = torch.Generator().manual_seed(seed)
            c["layers.0.act_fun.0.grid"].copy_(torch.sort(torch.rand(H, G + 1 + 2 * k, generator=g, dtype=torch.float64) * 4 - 2, dim=1).values)
    return net


def _layer_output(net, h):
    """y of the single KAN layer for rows h (the network up to the output Linear)."""
    v, c = net.views(), net.const_views()
    from ddr_amd.nn.kan import b_batch

    spline = torch.einsum("nij,ioj->nio", b_batch(h, c["layers.0.act_fun.0.grid"], net.k), v["layers.0.act_fun.0.coef"])
    y = v["layers.0.act_fun.0.scale_base"][None] * torch.nn.functional.silu(h)[:, :, None] + v["layers.0.act_fun.0.scale_sp"][None] * spline
    return (c["layers.0.act_fun.0.mask"][None] * y).sum(1)


@pytest.mark.parametrize("uniform", [True, False])
@pytest.mark.parametrize("G", [1, 3, 50])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_spline_identities_interior(k, G, uniform):
    H = 4
    net = _identity_net(H, G, k, uniform, seed=10 * G + k)
    t = net.const_views()["layers.0.act_fun.0.grid"]
    lo, hi = t[:, k], t[:, G + k]
    g = torch.Generator().manual_seed(3)
    w = torch.rand(200, H, generator=g, dtype=torch.float64) * (1 - 1e-9)
    h = lo[None] + w * (hi - lo)[None]  # in [t_k, t_{G+k})
    h[0] = lo  # the left end belongs to the interval
    coef = net.views()["layers.0.act_fun.0.coef"]
    with torch.no_grad():
        coef.fill_(1.0)  # partition of unity: sum_j B_j = 1 per input
        assert float((_layer_output(net, h) - H).abs().max()) <= 1e-12
        # Greville abscissae: sum_j mean(t_{j+1..j+k}) B_j(x) = x
        grev = torch.stack([t[:, j + 1:j + k + 1].mean(dim=1) for j in range(G + k)], dim=1)  # (H, G + k)
        coef.copy_(grev[:, None, :].expand(H, H, G + k))
        y = _layer_output(net, h)
        assert float((y - h.sum(1, keepdim=True)).abs().max()) <= 1e-12
        # the same through the module's own forward: u = sigmoid(W_out y + b_out)
        u = net(inputs=h)["u"]
        vv = net.views()
        ref = torch.sigmoid(y @ vv["output.weight"].t() + vv["output.bias"])[:, 0]
        assert float((u - ref).abs().max()) <= 1e-15


@pytest.mark.parametrize("uniform", [True, False])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_spline_identities_edges(k, uniform):
    H, G = 3, 5
    net = _identity_net(H, G, k, uniform, seed=k)
    t = net.const_views()["layers.0.act_fun.0.grid"]
    with torch.no_grad():
        net.views()["layers.0.act_fun.0.coef"].fill_(1.0)
        below = torch.stack([t[:, 0] - 1e-9, t[:, 0] - 5.0, torch.nextafter(t[:, 0], t[:, 0] - 1)])
        above = torch.stack([t[:, -1], t[:, -1] + 5.0, torch.nextafter(t[:, -1], t[:, -1] + 1)])
        for h in (below, above):  # h < t_0 and h >= t_last (the last knot itself: the interval is half-open)
            assert torch.equal(_layer_output(net, h), torch.zeros(3, H, dtype=torch.float64))
        y = _layer_output(net, t.t().contiguous())  # h at every knot
        assert bool(torch.isfinite(y).all())
        assert bool(torch.isfinite(net(inputs=t.t().contiguous())["u"]).all())


# the reference's tests/nn/test_kan.py, restated
def _ref_kan(num_hidden_layers=1):
    return TorchKan([f"attr_{i}" for i in range(5)], ["n", "q_spatial"], 11, num_hidden_layers, grid=3, k=3, seed=42,
                    device="cpu")


@pytest.mark.parametrize("layers", [1, 3])
def test_reference_cases(layers):
    model = _ref_kan(layers)
    x = torch.rand(10, 5, generator=torch.Generator().manual_seed(0))
    out = model(inputs=x)
    assert isinstance(out, dict) and set(out) == {"n", "q_spatial"}
    for key in ("n", "q_spatial"):
        assert out[key].shape == (10,)
        assert bool((out[key] >= 0).all()) and bool((out[key] <= 1).all())
    model.eval()
    with torch.no_grad():
        o1, o2 = model(inputs=x), model(inputs=x)
    assert torch.equal(o1["n"], o2["n"]) and torch.equal(o1["q_spatial"], o2["q_spatial"])
    (out["n"].sum() + out["q_spatial"].sum()).backward()
    assert any(p.grad is not None and bool((p.grad != 0).any()) for p in model.parameters())
    g = model.views(model.flat.grad)
    assert all(bool((g[k] != 0).any()) for k in ("input.weight", "layers.0.act_fun.0.coef", "output.bias"))


def test_initialisation_follows_the_published_scheme():
    net = TorchKan([f"a{i}" for i in range(10)], ["n"], 21, 2, 50, 2, seed=7)
    c, v = net.const_views(), net.views()
    t = c["layers.1.act_fun.0.grid"]
    assert t.shape == (21, 55) and abs(float(t[0, 0]) + 1.08) < 1e-6 and abs(float(t[0, -1]) - 1.08) < 1e-6
    assert bool((c["layers.0.act_fun.0.mask"] == 1).all()) and bool((c["layers.0.node_scale_0"] == 1).all())
    assert bool((c["layers.0.node_bias_0"] == 0).all())
    assert torch.allclose(v["layers.0.act_fun.0.scale_sp"], torch.full((21, 21), 1 / np.sqrt(21.0), dtype=torch.float32))
    assert float(v["layers.0.act_fun.0.scale_base"].detach().abs().max()) <= 1 / np.sqrt(21.0)
    # the fitted spline reproduces noise of the stated size at the grid points: |curve| <= 0.15 / G
    from ddr_amd.nn.kan import b_batch

    pts = t[:, 2:53].t().double()
    curve = torch.einsum("nij,ioj->nio", b_batch(pts, t.double(), 2), v["layers.0.act_fun.0.coef"].double())
    assert 0 < float(curve.abs().max()) <= 0.15 / 50 * (1 + 1e-4)
    same = TorchKan([f"a{i}" for i in range(10)], ["n"], 21, 2, 50, 2, seed=7)
    assert torch.equal(same.flat, net.flat)


def test_refusals():
    sd = {k: torch.from_numpy(v) for k, v in load_golden("kan_merit").items()}
    for cls in (TorchKan, kan):
        bad = dict(sd)
        bad["layers.1.symbolic_fun.0.mask"] = sd["layers.1.symbolic_fun.0.mask"].clone()
        bad["layers.1.symbolic_fun.0.mask"][3, 4] = 1.0
        with pytest.raises(RuntimeError, match="symbolic"):
            cls(**CKPT).load_state_dict(bad)
        bad = dict(sd)
        bad["layers.0.act_fun.0.grid"] = sd["layers.0.act_fun.0.grid"].clone()
        bad["layers.0.act_fun.0.grid"][5, 7] = bad["layers.0.act_fun.0.grid"][5, 6]
        with pytest.raises(RuntimeError, match="strictly increasing"):
            cls(**CKPT).load_state_dict(bad)
        bad = dict(sd)
        del bad["output.bias"]
        bad["extra"] = torch.zeros(1)
        with pytest.raises(RuntimeError, match="output.bias"):
            cls(**CKPT).load_state_dict(bad)
    # knots written in place are checked at the next call
    net = TorchKan(**CKPT)
    with torch.no_grad():
        net.const_views()["layers.0.act_fun.0.grid"][2, 10] = 5.0
    with pytest.raises(ValueError, match="strictly increasing"):
        net(inputs=torch.zeros(2, 10))
    # outside the fused path's envelope: refused at construction
    names = lambda n: [f"a{i}" for i in range(n)]  # noqa: E731
    for kw in (dict(input_var_names=names(33)), dict(hidden_size=33), dict(learnable_parameters=names(9)),
               dict(num_hidden_layers=5), dict(k=4), dict(k=0), dict(grid=0), dict(hidden_size=32, grid=30, k=3)):
        with pytest.raises(ValueError):
            kan(**{**CKPT, **kw})
    kan(**{**CKPT, **dict(hidden_size=32, grid=29, k=3)})  # the envelope's corner is inside
    # the fused path has no CPU fallback
    with pytest.raises(ValueError, match="device"):
        kan(**CKPT)(inputs=torch.zeros(2, 10))
