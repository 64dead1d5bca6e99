"""GPU parity of the fused C3 step tail (ddr_amd.train, csrc/train.hip) against the PyTorch ops it replaces:
the daily L1 objective + gradient (scripts/train.py:91-94) and clip_grad_norm_ + Adam (train.py:99-100).
Tolerances: the loss to 1e-6 relative (fp64 vs fp32 summation order), its gradient bitwise (sign x 1/count),
the parameters after five clipped Adam steps to 1e-6 relative (fused vs torch's operation order).

Against the float64 references of tail_cases.py (``l1_reference``, ``adam_reference``): the objective as above; for
clip + Adam the parameters, both moments (max-abs error over the largest reference entry) and the norm of every
step (relative) of the fused kernels K must be within MARGIN of the error of ``torch.optim.Adam`` +
``clip_grad_norm_`` in fp32 on the device T, on the same inputs (tail_cases.MARGIN, as in test_gpu_pnet.py; where
T's error is below one fp32 ulp, the 1e-6 above), and the short runs keep the 1e-6 as a ceiling.

Measured on an MI355X, 300 clipped steps at n = 4099 (err(T, R) / err(K, R)):
param 9.367e-07 / 9.367e-07; m 1.008e-07 / 8.938e-08; v 2.873e-06 / 2.269e-06; norm 7.601e-08 / 3.793e-08.
"""

import numpy as np
import pytest
import torch

import tail_cases as tc
from ddr_amd.train import ClipAdam, daily_l1_loss

pytestmark = pytest.mark.gpu

FIXED = 1e-6  # the bound where err(T, R) is below one fp32 ulp (tail_cases.bound)


@pytest.mark.parametrize("wd", [0, 5])
def test_daily_l1_matches_torch(cuda, wd):
    g = torch.Generator(device=cuda).manual_seed(3)
    daily = torch.rand((256, 89), device=cuda, generator=g).requires_grad_(True)
    obs = torch.rand((256, 89), device=cuda, generator=g)
    obs[3, 40] = daily[3, 40].detach()  # a zero difference: sign 0, as torch's abs backward
    loss = daily_l1_loss(daily, obs, wd)
    (loss * 2.0).backward()
    ref_in = daily.detach().clone().requires_grad_(True)
    ref = torch.nn.functional.l1_loss(ref_in[:, wd:], obs[:, wd:])
    (ref * 2.0).backward()
    assert abs(loss.item() - ref.item()) <= 1e-6 * abs(ref.item())
    torch.testing.assert_close(daily.grad, ref_in.grad, rtol=0, atol=0)
    assert float(daily.grad[:, :wd].abs().sum()) == 0.0


def test_daily_l1_rejects_cpu_and_bad_shapes(cuda):
    with pytest.raises(RuntimeError):
        daily_l1_loss(torch.zeros(2, 3), torch.zeros(2, 3), 0)
    with pytest.raises(ValueError):
        daily_l1_loss(torch.zeros(2, 3, device=cuda), torch.zeros(2, 4, device=cuda), 0)


@pytest.mark.parametrize("scale", [1e-3, 10.0], ids=["unclipped", "clipped"])
def test_clip_adam_matches_torch(cuda, scale):
    torch.manual_seed(0)
    p0 = torch.randn(34179, device=cuda)
    ours = p0.clone()
    ref = torch.nn.Parameter(p0.clone())
    opt = ClipAdam(ours, lr=1e-3, max_norm=1.0)
    topt = torch.optim.Adam([ref], lr=1e-3)
    for k in range(5):
        grad = torch.randn(p0.shape, device=cuda, generator=torch.Generator(device=cuda).manual_seed(k)) * scale
        ours.grad = grad.clone()
        ref.grad = grad.clone()
        opt.step()
        norm = torch.nn.utils.clip_grad_norm_([ref], max_norm=1.0)
        topt.step()
        assert abs(opt.last_norm.item() - norm.item()) <= 1e-6 * norm.item()
    err = (ours - ref.detach()).abs().max().item()
    assert err <= 1e-6 * ref.detach().abs().max().item(), err
    np.testing.assert_array_equal(opt.m.cpu().numpy() != 0, np.ones(p0.shape, bool))


# ---------------------------------------------------------------------------------- daily L1 against float64


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def l1_expected_grad(daily, obs, warmup, inv_count=None, upstream=1.0) -> np.ndarray:
    """float32(sign inv_count) (times a float32 upstream factor, rounded once more), 0 before the warm-up."""
    G, D = daily.shape
    inv = np.float32(1.0 / (G * (D - warmup)) if inv_count is None else inv_count)
    _, g = tc.l1_reference(daily.numpy(), obs.numpy(), warmup, 1.0)
    return (g.astype(np.float32) * inv) * np.float32(upstream)


@pytest.mark.parametrize("G,D,warmup", tc.L1_SHAPES)
def test_daily_l1_against_float64(cuda, G, D, warmup):
    daily, obs = tc.l1_inputs(G, D, warmup)
    ref, _ = tc.l1_reference(daily.numpy(), obs.numpy(), warmup)
    d = daily.to(cuda).requires_grad_(True)
    loss = daily_l1_loss(d, obs.to(cuda), warmup)
    loss.backward()
    assert loss.shape == () and abs(loss.item() - ref) <= 1e-6 * abs(ref), (loss.item(), ref)
    want = l1_expected_grad(daily, obs, warmup)
    got = d.grad.cpu().numpy()
    assert got.shape == want.shape and (bits(got) == bits(want)).all()
    assert not got[:, :warmup].any()


def test_daily_l1_interfaces(cuda):
    G, D, warmup = 37, 53, 4
    daily, obs = tc.l1_inputs(G, D, warmup)
    obs_d = obs.to(cuda)
    base = daily_l1_loss(daily.to(cuda), obs_d, warmup)  # daily needs no gradient: the kernel gets no grad pointer
    ref, _ = tc.l1_reference(daily.numpy(), obs.numpy(), warmup)
    assert not base.requires_grad and abs(base.item() - ref) <= 1e-6 * abs(ref)
    # an explicit inv_count that is not the mean's
    d = daily.to(cuda).requires_grad_(True)
    loss = daily_l1_loss(d, obs_d, warmup, inv_count=0.37)
    loss.backward()
    ref37, _ = tc.l1_reference(daily.numpy(), obs.numpy(), warmup, 0.37)
    assert abs(loss.item() - ref37) <= 1e-6 * abs(ref37)
    assert (bits(d.grad.cpu().numpy()) == bits(l1_expected_grad(daily, obs, warmup, 0.37))).all()
    # the same loss value with and without a gradient
    d = daily.to(cuda).requires_grad_(True)
    with_grad = daily_l1_loss(d, obs_d, warmup)
    assert with_grad.requires_grad and with_grad.item() == base.item()
    # an upstream factor
    (with_grad * 3.0).backward()
    assert (bits(d.grad.cpu().numpy()) == bits(l1_expected_grad(daily, obs, warmup, upstream=3.0))).all()
    # a transposed view as the leaf: the gradient arrives in its layout
    dt = daily.t().contiguous().to(cuda).t().requires_grad_(True)
    assert dt.shape == (G, D) and not dt.is_contiguous() and dt.is_leaf
    loss = daily_l1_loss(dt, obs_d, warmup)
    loss.backward()
    assert loss.item() == base.item()
    assert dt.grad.shape == (G, D)
    assert (bits(dt.grad.cpu().numpy()) == bits(l1_expected_grad(daily, obs, warmup))).all()
    # ... and a transposed view of a leaf
    leaf = daily.t().contiguous().to(cuda).requires_grad_(True)  # (D, G)
    daily_l1_loss(leaf.t(), obs_d, warmup).backward()
    assert (bits(leaf.grad.cpu().numpy()) == bits(l1_expected_grad(daily, obs, warmup).T)).all()


def test_daily_l1_propagates_nan(cuda):
    """A NaN difference after the warm-up makes the loss NaN and the gradient NaN at exactly that element (every
    other element keeps sign x 1/count); inside the warm-up it changes nothing.  PyTorch's ``abs`` backward gives 0
    at that element (sgn(NaN) = 0) under a NaN loss; the kernel marks the element instead.  The reference loop never
    reaches either: scripts/train.py:84-92 drops the gauges whose observations hold a NaN before the loss."""
    G, D, warmup = 37, 53, 4
    daily, obs = tc.l1_inputs(G, D, warmup)
    want = l1_expected_grad(daily, obs, warmup)
    clean = daily_l1_loss(daily.to(cuda), obs.to(cuda), warmup).item()
    for at, live in (((5, 20), True), ((5, warmup), True), ((5, warmup - 1), False)):
        o = obs.clone()
        o[at] = float("nan")
        d = daily.to(cuda).requires_grad_(True)
        loss = daily_l1_loss(d, o.to(cuda), warmup)
        loss.backward()
        got = d.grad.cpu().numpy()
        if live:
            assert np.isnan(loss.item())
            assert np.isnan(got[at]) and int(np.isnan(got).sum()) == 1
            keep = np.ones((G, D), bool)
            keep[at] = False
            assert (bits(got)[keep] == bits(want)[keep]).all()
        else:
            assert loss.item() == clean
            assert (bits(got) == bits(want)).all()


# -------------------------------------------------------------------------------- clip + Adam against float64


def run_clip_adam(cuda, p0, grads, lr, betas, eps, max_norm):
    """The fused optimizer over ``grads``: (params, m, v, norms) as float64 NumPy, and the optimizer."""
    p = p0.to(cuda).clone()
    opt = ClipAdam(p, lr=lr, betas=betas, eps=eps, max_norm=max_norm)
    norms = []
    for g in grads:
        p.grad = g.to(cuda)
        opt.step()
        norms.append(float(opt.last_norm))
    f = lambda t: t.double().cpu().numpy()  # noqa: E731
    return (f(p), f(opt.m), f(opt.v), norms), opt


def adam_errors(got, ref):
    out = {}
    for name, a, r in zip(("param", "m", "v"), got, ref):
        assert np.isfinite(a).all(), name
        out[name] = float(np.abs(a - r).max() / max(np.abs(r).max(), 1e-300))
    out["norm"] = max(abs(a - r) / max(r, 1e-300) for a, r in zip(got[3], ref[3]))
    return out


def check_adam(cuda, n, steps, scale, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_norm=1.0, ceiling=True, seed=0):
    p0 = torch.randn(n, generator=torch.Generator().manual_seed(n + 1))
    grads = tc.adam_grads(n, steps, scale, seed)
    ref = tc.adam_reference(p0.numpy(), [g.numpy() for g in grads], lr, betas, eps, max_norm)
    et = adam_errors(tc.torch_adam(p0.to(cuda), grads, lr, betas, eps, max_norm), ref)
    got, opt = run_clip_adam(cuda, p0, grads, lr, betas, eps, max_norm)
    ek = adam_errors(got, ref)
    failed = []
    for name in ("param", "m", "v", "norm"):
        t, k = et[name], ek[name]
        bound = tc.bound(t, FIXED)
        if ceiling and name == "param":
            bound = min(bound, 1e-6)
        print(f"adam n={n} steps={steps} scale={scale} betas={betas} eps={eps} max_norm={max_norm} {name}: "
              f"T {t:.3e} K {k:.3e} ratio {k / t if t > 0 else float('nan'):.2f}")
        if not k <= bound:
            failed.append((name, t, k, bound))
    assert not failed, failed
    assert float(opt.step_count) == steps
    return ref, got, opt


@pytest.mark.parametrize("clipped", [True, False], ids=["clipped", "unclipped"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 16383, 16384, 16385, 34179, 1_000_003])
def test_clip_adam_lengths(cuda, n, clipped):
    """One element, either side of a workgroup (256) and of the grid (64 x 256 = 16384: below it some workgroups
    are empty, above it threads take a second element), the network's 34179 and more than a million."""
    ref, _, _ = check_adam(cuda, n, 3, 100.0 if clipped else 1e-4)
    assert all((norm > 1.0) == clipped for norm in ref[3]), ref[3]


@pytest.mark.parametrize("max_norm", [0.0, -1.0])
def test_clip_adam_without_clipping(cuda, max_norm):
    ref, got, opt = check_adam(cuda, 4099, 3, 100.0, max_norm=max_norm)
    assert ref[3][-1] > 1000.0 and abs(float(opt.last_norm) - ref[3][-1]) <= 1e-6 * ref[3][-1]
    # unclipped indeed: the first moment is of the gradient's size
    assert np.abs(got[1]).max() > 10.0


def test_clip_adam_zero_gradient(cuda):
    """norm 0, v = 0, den = eps: parameters and moments unchanged and finite."""
    n = 4099
    p0 = torch.randn(n, generator=torch.Generator().manual_seed(2))
    got, opt = run_clip_adam(cuda, p0, [torch.zeros(n)], 1e-3, (0.9, 0.999), 1e-8, 1.0)
    assert np.array_equal(got[0], p0.double().numpy())
    assert not got[1].any() and not got[2].any() and got[3] == [0.0]
    assert float(opt.step_count) == 1.0
    # and the next step is the reference's second step
    g = tc.adam_grads(n, 1, 100.0)[0]
    opt.param.grad = g.to(cuda)
    opt.step()
    grads = [torch.zeros(n), g]
    ref = tc.adam_reference(p0.numpy(), [t.numpy() for t in grads])
    et = adam_errors(tc.torch_adam(p0.to(cuda), grads), ref)
    f = lambda t: t.double().cpu().numpy()  # noqa: E731
    ek = adam_errors((f(opt.param), f(opt.m), f(opt.v), [0.0, float(opt.last_norm)]), ref)
    for name in ("param", "m", "v", "norm"):
        print(f"adam after a zero gradient {name}: T {et[name]:.3e} K {ek[name]:.3e}")
        assert ek[name] <= tc.bound(et[name], FIXED), (name, et[name], ek[name])
    assert ek["param"] <= 1e-6


def test_clip_adam_other_betas_and_eps(cuda):
    check_adam(cuda, 4099, 3, 100.0, betas=(0.5, 0.9), eps=1e-3)
    check_adam(cuda, 4099, 3, 1e-4, betas=(0.5, 0.9), eps=1e-3)


def test_clip_adam_300_steps(cuda):
    """Long enough for the fp32 step counter and the bias corrections' pow to matter (beta2^300 = 0.74)."""
    check_adam(cuda, 4099, 300, 100.0, ceiling=False)


def test_clip_adam_bookkeeping(cuda):
    """``.grad`` stays the unclipped gradient that was set, the device step counter counts the steps, and a step
    without a gradient changes nothing."""
    n = 4099
    p = torch.randn(n, generator=torch.Generator().manual_seed(3)).to(cuda)
    opt = ClipAdam(p, lr=1e-3, max_norm=1.0)
    for k, g in enumerate(tc.adam_grads(n, 3, 100.0), 1):
        p.grad = g.to(cuda)
        opt.step()
        assert float(opt.last_norm) > 1.0  # clipped
        assert torch.equal(p.grad.cpu(), g) and (bits(p.grad.cpu().numpy()) == bits(g.numpy())).all()
        assert float(opt.step_count) == k
    before = [t.clone() for t in (p, opt.m, opt.v, opt.step_count, opt.last_norm)]
    opt.zero_grad()
    assert p.grad is None
    opt.step()
    for a, b in zip(before, (p, opt.m, opt.v, opt.step_count, opt.last_norm)):
        assert torch.equal(a, b)
