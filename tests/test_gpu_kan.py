"""The fused KAN (csrc/kan.hip; the reference's src/ddr/nn/kan.py:11-62) against ``TorchKan`` in fp64 on the CPU.

Bars (measured in the test, not fixed): with e32 the error of ``TorchKan`` run in fp32 ON THE GPU against the
same fp64 model on the same inputs, the outputs' max-abs error is at most max(4 e32, 2e-7) and each trainable
tensor's gradient norm-rel error at most max(4 e32, 1e-6); the factor 4 covers a different summation order and the
device's exp and divide in SiLU and sigmoid.  A tensor whose fp64 gradient is entirely zero is compared by
max-abs <= 1e-12.  Inputs are randn x 3, so a large share of every layer's inputs lies outside the knots (only the
SiLU branch live).  Every figure is printed (``pytest -s``).  Parity with pykan itself is not pinned."""

import ctypes as C

import pytest
import torch

from conftest import load_golden
from ddr_amd import _lib
from ddr_amd.nn import TorchKan, kan, load_checkpoint
from ddr_amd.train import ClipAdam

pytestmark = pytest.mark.gpu

PARAMS = ["n", "q_spatial", "p_spatial", "p4", "p5", "p6", "p7", "p8"]


def build(cls, F, H, L, G, k, O, device="cpu", seed=0):
    return cls([f"a{i}" for i in range(F)], PARAMS[:O], H, L, G, k, seed, device=device)


def merit_state():
    return {k: torch.from_numpy(v) for k, v in load_golden("kan_merit").items()}


def trio(cuda, F, H, L, G, k, O, setup=None):
    """(fused on the GPU, TorchKan fp32 on the GPU, TorchKan fp64 on the CPU) with the same parameters."""
    model = build(TorchKan, F, H, L, G, k, O)
    if setup is not None:
        setup(model)
    fused, t32 = build(kan, F, H, L, G, k, O, device=cuda), build(TorchKan, F, H, L, G, k, O, device=cuda)
    for net in (fused, t32):
        with torch.no_grad():
            net.flat.copy_(model.flat)
            net.consts.copy_(model.consts)
    return fused, t32, model.double()


def load_merit(model):
    model.load_state_dict(merit_state())


def randomise(model):
    """Random weights, sorted-random knots (different per row), a mask with 30 % zeros, non-trivial node and
    subnode scale and bias."""
    g = torch.Generator().manual_seed(11)
    v, c = model.views(), model.const_views()
    with torch.no_grad():
        for name, t in v.items():
            if name.endswith("coef"):
                t.copy_(torch.randn(t.shape, generator=g) * 0.2)
            elif name.endswith("scale_sp"):
                t.copy_(torch.rand(t.shape, generator=g) * 0.3 + 0.1)
            elif name.endswith("scale_base"):
                t.copy_(torch.randn(t.shape, generator=g) * 0.3)
            elif name.endswith("bias"):
                t.copy_(torch.randn(t.shape, generator=g) * 0.1)
        for name, t in c.items():
            if name.endswith("grid"):
                t.copy_(torch.sort(torch.rand(t.shape, generator=g) * 3 - 1.5, dim=1).values)
                assert bool((t[:, 1:] > t[:, :-1]).all())
            elif name.endswith("mask"):
                t.copy_((torch.rand(t.shape, generator=g) >= 0.3).float())
            elif name.endswith("scale_0"):
                t.copy_(torch.rand(t.shape, generator=g) + 0.5)
            else:
                t.copy_(torch.randn(t.shape, generator=g) * 0.1)


def run(net, x, w, chunk=None):
    """u (N, O) and dL/dflat for L = sum u w; in chunks of rows (the gradient of a sum adds up)."""
    net.flat.grad = None
    outs = []
    for s in range(0, x.shape[0], chunk or x.shape[0]):
        o = net(inputs=x[s:s + (chunk or x.shape[0])])
        u = torch.stack([o[k] for k in net.learnable_parameters], dim=1)
        (u * w[s:s + u.shape[0]]).sum().backward()
        outs.append(u.detach())
    return torch.cat(outs), net.flat.grad.detach().clone()


def normrel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def check_parity(cuda, fused, t32, t64, x, tag):
    """The issue's bars; returns the fused outputs."""
    g = torch.Generator().manual_seed(5)
    w = torch.randn(x.shape[0], t64.output_size, generator=g)
    u64, g64 = run(t64, x.double(), w.double(), chunk=2048)
    u32, g32 = run(t32, x.to(cuda), w.to(cuda))
    uf, gf = run(fused, x.to(cuda), w.to(cuda))
    e32 = float((u32.cpu().double() - u64).abs().max())
    ef = float((uf.cpu().double() - u64).abs().max())
    print(f"[{tag}] N={x.shape[0]} output max-abs: fused {ef:.2e}  TorchKan fp32 {e32:.2e}  bar {max(4 * e32, 2e-7):.2e}")
    failures = []
    if not ef <= max(4 * e32, 2e-7):
        failures.append(("output", ef, e32))
    v64, v32, vf = t64.views(g64), t32.views(g32.cpu()), fused.views(gf.cpu())
    for name, ref in v64.items():
        if not bool((ref != 0).any()):
            err = float(vf[name].double().abs().max())
            print(f"[{tag}]   grad {name}: fp64 gradient all zero, fused max-abs {err:.2e}")
            if not err <= 1e-12:
                failures.append((name, err, 0.0))
            continue
        e32g, efg = normrel(v32[name], ref), normrel(vf[name], ref)
        print(f"[{tag}]   grad {name}: fused {efg:.2e}  TorchKan fp32 {e32g:.2e}  bar {max(4 * e32g, 1e-6):.2e}")
        if not efg <= max(4 * e32g, 1e-6):
            failures.append((name, efg, e32g))
    assert bool(torch.isfinite(gf).all())
    assert not failures, failures
    return uf


def inputs(N, F, seed=0):
    return torch.randn(N, F, generator=torch.Generator().manual_seed(seed)) * 3


@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, 70001])
def test_parity_published_weights(cuda, N):
    """N = 70001: a workgroup takes more than one tile and more than one partial is reduced."""
    fused, t32, t64 = trio(cuda, 10, 21, 2, 50, 2, 3, load_merit)
    check_parity(cuda, fused, t32, t64, inputs(N, 10, seed=N), f"merit N={N}")


@pytest.mark.parametrize("arch", [(5, 11, 3, 3, 3, 2), (1, 1, 1, 1, 1, 1), (32, 32, 1, 29, 3, 8)],
                         ids=lambda a: "-".join(map(str, a)))
def test_parity_architectures(cuda, arch):
    F, H, L, G, k, O = arch
    fused, t32, t64 = trio(cuda, F, H, L, G, k, O)
    check_parity(cuda, fused, t32, t64, inputs(257, F, seed=H), f"arch {arch}")


def test_parity_random_weights_knots_mask(cuda):
    fused, t32, t64 = trio(cuda, 10, 21, 2, 50, 2, 3, randomise)
    check_parity(cuda, fused, t32, t64, inputs(257, 10, seed=9), "random weights, knots, mask")


@pytest.mark.parametrize("k", [1, 2, 3])
def test_knots_and_edges(cuda, k):
    """F = H with the identity input Linear, so h^0 = x: rows at every stored fp32 knot, its neighbours in both
    directions, and +-8.  Rows below t_0 or at / above t_last equal the SiLU-only value."""
    H, G = 8, 5

    def setup(model):
        v = model.views()
        with torch.no_grad():
            v["input.weight"].copy_(torch.eye(H))
            v["input.bias"].zero_()
            v["layers.0.act_fun.0.coef"].mul_(50.0)  # a spline branch as large as the SiLU branch

    fused, t32, t64 = trio(cuda, H, H, 1, G, k, 2, setup)
    t = t64.const_views()["layers.0.act_fun.0.grid"][0].float()  # uniform: the same row for every input
    vals = torch.cat([t, torch.nextafter(t, t - 1), torch.nextafter(t, t + 1), torch.tensor([-8.0, 8.0])])
    x = vals[:, None].expand(-1, H).contiguous()
    uf = check_parity(cuda, fused, t32, t64, x, f"knots k={k}")
    outside = (vals < t[0]) | (vals >= t[-1])
    assert int(outside.sum()) == 5 and bool(outside[len(t) - 1])  # the last knot itself is outside
    silu_only = build(TorchKan, H, H, 1, G, k, 2).double()
    with torch.no_grad():
        silu_only.flat.copy_(t64.flat)
        silu_only.consts.copy_(t64.consts)
        silu_only.views()["layers.0.act_fun.0.coef"].zero_()
        o = silu_only(inputs=x.double())
        ref = torch.stack([o[p] for p in silu_only.learnable_parameters], dim=1)
        e32 = t32(inputs=x.to(cuda))
        e32 = float((torch.stack([e32[p] for p in t32.learnable_parameters], dim=1).cpu().double() - ref)[outside].abs().max())
    err = float((uf.cpu().double() - ref)[outside].abs().max())
    print(f"[knots k={k}] outside rows vs SiLU-only: fused {err:.2e}  TorchKan fp32 {e32:.2e}")
    assert err <= max(4 * e32, 2e-7)
    inside = ~outside
    assert float((uf.cpu().double() - ref)[inside].abs().max()) > 1e-4  # (the spline branch is live inside)


def test_determinism(cuda):
    fused, _, _ = trio(cuda, 10, 21, 2, 50, 2, 3, load_merit)
    x = inputs(50000, 10, seed=2).to(cuda)
    w = torch.randn(50000, 3, generator=torch.Generator().manual_seed(6)).to(cuda)
    u1, g1 = run(fused, x, w)
    u2, g2 = run(fused, x, w)
    assert torch.equal(u1, u2) and torch.equal(g1, g2)
    assert bool(torch.isfinite(g1).all()) and bool((g1 != 0).any())


def test_checkpoint_round_trip(cuda, tmp_path):
    sd = merit_state()
    path = tmp_path / "ckpt.pt"
    torch.save({"model_state_dict": {k: v.clone() for k, v in sd.items()}, "epoch": 3, "mini_batch": 7}, path)
    net = build(kan, 10, 21, 2, 50, 2, 3, device=cuda)
    state = load_checkpoint(net, path, cuda)
    assert state["epoch"] == 3 and state["mini_batch"] == 7
    out = {k: v.cpu() for k, v in net.state_dict().items()}
    assert list(out) == list(sd) and all(torch.equal(out[k], sd[k]) for k in sd)
    N = 1000
    with torch.no_grad():
        o = net(inputs=inputs(N, 10).to(cuda))
    assert list(o) == ["n", "q_spatial", "p_spatial"] and o["n"].shape == (N,)
    assert all(bool((v >= 0).all()) and bool((v <= 1).all()) for v in o.values())
    # the second published checkpoint evaluates too
    net.load_state_dict({k: torch.from_numpy(v) for k, v in load_golden("kan_lynker").items()})
    with torch.no_grad():
        o = net(inputs=inputs(N, 10).to(cuda))
    assert all(v.shape == (N,) and bool((v >= 0).all()) and bool((v <= 1).all()) for v in o.values())


def test_training_hook(cuda):
    """Three ClipAdam steps on the one flat parameter lower sum (u - 0.3)^2; no buffer changes."""
    fused, _, _ = trio(cuda, 10, 21, 2, 50, 2, 3, load_merit)
    x = inputs(2000, 10, seed=4).to(cuda)
    opt = ClipAdam(fused.flat)
    consts = fused.consts.clone()
    losses = []
    for _ in range(4):
        o = fused(inputs=x)
        loss = sum(((v - 0.3) ** 2).sum() for v in o.values())
        losses.append(loss.item())
        opt.zero_grad()
        loss.backward()
        opt.step()
    print("[training hook] losses", losses)
    assert losses[3] < losses[2] < losses[1] < losses[0]
    assert torch.equal(fused.consts, consts)


def test_refusals(cuda):
    net = build(kan, 10, 21, 2, 50, 2, 3, device=cuda)
    x = inputs(8, 10)
    with pytest.raises(ValueError):
        net(inputs=x)  # host inputs
    with pytest.raises(ValueError):
        net(inputs=x.to(cuda).requires_grad_(True))
    with torch.no_grad():  # (no gradient asked for: fine)
        net(inputs=x.to(cuda).requires_grad_(True))
    with pytest.raises(ValueError):
        build(kan, 10, 21, 2, 50, 2, 3, device=cuda).double()(inputs=x.to(cuda))
    with pytest.raises(ValueError):
        build(kan, 10, 21, 2, 50, 2, 3)(inputs=x.to(cuda))  # parameters on the host
    # an out-of-envelope descriptor straight to the C ABI: refused before any pointer is used
    lib = _lib.load()
    for bad, word in ((dict(hidden=33), "hidden"), (dict(k=4), "k"), (dict(n_features=0), "n_features"),
                      (dict(hidden=32, grid=30, k=3), "32768")):
        d = _lib.KanDesc(**{**dict(n_features=10, hidden=21, n_outputs=3, n_layers=2, grid=50, k=2), **bad})
        assert lib.ddr_kan_forward_f32(C.byref(d), 8, None, None, None, None, None, None, None) == _lib.DDR_ERR_ARG
        assert word in lib.ddr_last_error().decode()
        assert lib.ddr_kan_backward_f32(C.byref(d), 8, None, None, None, None, None, None, None, None, None) == _lib.DDR_ERR_ARG
        assert int(lib.ddr_kan_param_count(C.byref(d))) == -1
        with pytest.raises(_lib.DDRError):
            _lib.check(lib.ddr_kan_forward_f32(C.byref(d), 8, None, None, None, None, None, None, None))
    good = _lib.KanDesc(10, 21, 3, 2, 50, 2)
    assert int(lib.ddr_kan_param_count(C.byref(good))) == 47925 == net.flat.numel()
    assert int(lib.ddr_kan_const_count(C.byref(good))) == net.consts.numel()
    assert lib.ddr_kan_forward_f32(C.byref(good), 0, None, None, None, None, None, None, None) == _lib.DDR_ERR_ARG


def test_no_grad_inference_is_bitwise(cuda):
    fused, _, _ = trio(cuda, 10, 21, 2, 50, 2, 3, load_merit)
    x = inputs(300000, 10, seed=8).to(cuda)
    o1 = fused(inputs=x)
    with torch.no_grad():
        o2 = fused(inputs=x)
    assert o1["n"].requires_grad and not o2["n"].requires_grad
    assert all(torch.equal(o1[k].detach(), o2[k]) for k in o1)
