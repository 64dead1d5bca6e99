"""The float64 references and case generators of tests/tail_cases.py, checked without a GPU: the GPU tests of the
C3 step tail (test_gpu_pnet.py, test_gpu_train.py) rest on them."""

import numpy as np
import pytest
import torch

import tail_cases as tc
from ddr_amd.pnet import param_count


@pytest.mark.parametrize("scale,max_norm,betas,eps", [
    (10.0, 1.0, (0.9, 0.999), 1e-8),   # clipped
    (1e-3, 1.0, (0.9, 0.999), 1e-8),   # unclipped
    (1.0, 0.0, (0.9, 0.999), 1e-8),    # clipping off
    (0.0, 1.0, (0.9, 0.999), 1e-8),    # zero gradients
    (10.0, 1.0, (0.5, 0.9), 1e-3),     # non-default betas and eps
], ids=["clipped", "unclipped", "off", "zero", "betas"])
def test_adam_reference_matches_torch_float64(scale, max_norm, betas, eps):
    n = 4099
    p0 = torch.randn(n, generator=torch.Generator().manual_seed(5)).double()
    grads = [g.double() for g in tc.adam_grads(n, 7, scale)]
    ref = tc.adam_reference(p0.numpy(), [g.numpy() for g in grads], 1e-3, betas, eps, max_norm)
    got = tc.torch_adam(p0, grads, 1e-3, betas, eps, max_norm)
    for name, a, b in zip(("param", "m", "v"), ref, got):
        assert np.abs(a - b).max() <= 1e-12 * max(np.abs(b).max(), 1e-300), name
    np.testing.assert_allclose(ref[3], got[3], rtol=1e-12, atol=0)
    if scale == 0.0:
        assert np.array_equal(ref[0], p0.numpy()) and not ref[1].any() and not ref[2].any()


@pytest.mark.parametrize("G,D,warmup", tc.L1_SHAPES)
def test_l1_reference_matches_torch_float64(G, D, warmup):
    daily, obs = tc.l1_inputs(G, D, warmup)
    diff = (daily - obs)[:, warmup:]
    assert (diff == 0).any()
    if diff.numel() > 1:
        assert (diff > 0).any() and (diff < 0).any()
    loss, grad = tc.l1_reference(daily.numpy(), obs.numpy(), warmup)
    d64 = daily.double().requires_grad_(True)
    ref = torch.nn.functional.l1_loss(d64[:, warmup:], obs.double()[:, warmup:])
    ref.backward()
    assert abs(loss - ref.item()) <= 1e-13 * abs(ref.item())
    np.testing.assert_allclose(grad, d64.grad.numpy(), rtol=1e-15, atol=0)
    assert not grad[:, :warmup].any()
    loss3, grad3 = tc.l1_reference(daily.numpy(), obs.numpy(), warmup, inv_count=3.0)
    count = G * (D - warmup)
    assert abs(loss3 - 3.0 * count * ref.item()) <= 1e-13 * abs(loss3)
    np.testing.assert_array_equal(grad3, 3.0 * np.sign(grad))


def test_pnet_reference_gradient_matches_finite_differences():
    """Central differences (step 1e-6, float64) on three entries of each of the eight blocks."""
    F, N, h = 5, 17, 1e-6
    table = tc.TABLES["default"]  # p_spatial in log space
    flat = tc.make_params(F).double().numpy()
    x = tc.make_inputs("plain", N, F)
    gouts = tc.make_gouts(N)
    net = tc._torch_net(F, table, flat).double()
    with torch.no_grad():
        net.flat.copy_(torch.from_numpy(flat))  # the float64 values themselves, not their fp32 rounding
    tc.weighted_loss(net(x.double()), gouts).backward()
    grad = net.flat.grad.numpy()
    # pnet_reference computes the same gradient from the fp32 parameters
    _, g32 = tc.pnet_reference(F, table, flat.astype(np.float32), x, gouts)
    assert tc.errors(g32, grad)[0] <= 1e-6

    def loss_at(p):
        with torch.no_grad():
            net.flat.copy_(torch.from_numpy(p))
            return float(tc.weighted_loss(net(x.double()), gouts))

    rng = np.random.default_rng(0)
    o = 0
    for name, shp in tc.block_shapes(F):
        k = int(np.prod(shp))
        for e in rng.choice(k, 3, replace=False):
            p = flat.copy()
            p[o + e] += h
            up = loss_at(p)
            p[o + e] -= 2 * h
            fd = (up - loss_at(p)) / (2 * h)
            assert abs(fd - grad[o + e]) <= 1e-6 * abs(grad[o + e]), (name, int(e), fd, grad[o + e])
        o += k
    assert o == param_count(F)


def test_blocks_and_errors():
    F = 3
    ref = np.arange(1, param_count(F) + 1, dtype=np.float64)
    b = tc.blocks(ref, F)
    assert list(b) == list(tc.BLOCKS)
    assert b["w1"].shape == (128, F) and b["w4"].shape == (3, 128) and b["b4"].shape == (3,)
    assert b["b1"][0] == 128 * F + 1 and b["b4"][-1] == param_count(F)
    a = ref.copy()
    a[128 * F + 5] += 1.0  # one element of b1
    e = tc.block_errors(a, ref, F)
    assert e["b1"][1] == 1.0 / b["b1"].max() and e["b1"][0] > 0
    assert all(e[k] == (0.0, 0.0) for k in tc.BLOCKS if k != "b1")
    # a zero reference block must be met exactly
    z = ref.copy()
    z[:128 * F] = 0
    assert tc.block_errors(z, z, F)["w1"] == (0.0, 0.0)
    a = z.copy()
    a[7] = 1e-30
    assert tc.block_errors(a, z, F)["w1"] == (np.inf, np.inf)
    a = ref.copy()
    a[-1] = np.nan
    assert tc.block_errors(a, ref, F)["b4"] == (np.inf, np.inf)


@pytest.mark.parametrize("N", [64, 130])
def test_saturating_case_saturates(N):
    """Conditions on the float64 reference alone: SiLU saturated on both sides, U within 1e-4 of 0 and of 1, and
    everything finite."""
    F = 10
    flat = tc.make_params(F)
    x = tc.make_inputs("saturating", N, F)
    z, u = tc.pnet_internals(F, flat, x)
    assert (z < -20).mean() >= 0.01 and (z > 20).mean() >= 0.01
    for l in range(3):  # every hidden layer takes part
        assert (z[l] < -20).any() and (z[l] > 20).any()
    lo, hi = (u < 1e-4).mean(), (u > 1 - 1e-4).mean()
    assert lo + hi >= 0.05 and lo > 0 and hi > 0
    for name in tc.TABLES:
        outs, grad = tc.pnet_reference(F, tc.TABLES[name], flat, x, tc.make_gouts(N))
        assert all(np.isfinite(o).all() for o in outs) and np.isfinite(grad).all()
        assert all(np.abs(v).max() > 0 for v in tc.blocks(grad, F).values())


def test_input_generators():
    x = tc.make_inputs("constant_tile", 130, 10)
    assert (x[64:128] == x[64]).all() and not (x[:64] == x[0]).all() and not (x[128] == x[64]).all()
    x = tc.make_inputs("constant_tile", 64, 10)
    assert (x == x[0]).all()
    assert not tc.make_inputs("zeros", 130, 4).any()
    assert torch.equal(tc.make_inputs("plain", 17, 3), tc.make_inputs("plain", 17, 3))
    g = tc.make_gouts(130, row=64)
    assert all(int((t != 0).sum()) == 1 and t[64] != 0 for t in g)
    g = tc.make_gouts(130, only=1)
    assert g[0] is None and g[2] is None and g[1].shape == (130,)
    # x = 0: the reference's dW1 is identically zero
    _, grad = tc.pnet_reference(4, tc.TABLES["default"], tc.make_params(4), tc.make_inputs("zeros", 130, 4),
                                tc.make_gouts(130))
    assert not tc.blocks(grad, 4)["w1"].any() and tc.blocks(grad, 4)["b1"].any()
    # N = 0
    outs, grad = tc.pnet_reference(4, tc.TABLES["default"], tc.make_params(4), torch.zeros((0, 4)), tc.make_gouts(0))
    assert all(o.shape == (0,) for o in outs) and not grad.any()
