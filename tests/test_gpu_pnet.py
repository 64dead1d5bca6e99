"""The fused parameter network (csrc/pnet.hip; C3's stand-in for the reference's KAN, src/ddr/nn/kan.py:11-62)
against the same network in PyTorch ops (fp32, hipBLASLt GEMMs + autograd), and against that network in float64 on
the CPU (tail_cases.pnet_reference).

Tolerances: outputs max-rel 1e-5 (fp32 GEMMs summed in another order: ~1e-7 per product chain, amplified at most
by the log-space denormalisation's exp); parameter gradients norm-relative 1e-5.

The float64 comparisons (``check``) have no fixed tolerance: with R the float64 reference, T the PyTorch network in
fp32 on the device and K the fused kernels, all on the same fp32 parameters, inputs and output gradients, each of
the three outputs (max-rel, floor 1e-6) and each of the eight parameter-gradient blocks (norm-relative and
max-abs over the block's largest reference entry) must satisfy err(K, R) <= MARGIN err(T, R)
(tail_cases.MARGIN).  Both fp32 paths amplify rounding alike where the network saturates (u (1 - u) from an fp32 u
next to 1), so the bound follows the case.  Where err(T, R) is below one fp32 ulp (2^-23: T is right to the last bit of the block's largest entry, as
happens with one row, three entries or an identically zero block) the ratio says nothing and the bound is the 1e-5
above.  MARGIN and the measured errors: DESIGN.md section 5.
"""

import functools

import numpy as np
import pytest
import torch

import tail_cases as tc
from conftest import normrel
from ddr_amd.pnet import ParamNet, TorchParamNet, param_count

pytestmark = pytest.mark.gpu

RANGES = {"n": [0.015, 0.25], "q_spatial": [0.0, 1.0], "p_spatial": [1.0, 200.0]}

FIXED = 1e-5  # the bound where err(T, R) is below one fp32 ulp (tail_cases.bound)


@pytest.mark.parametrize("N,F", [(1, 10), (63, 10), (1000, 7), (70001, 10), (300000, 10)])
def test_fused_network_matches_torch(cuda, N, F):
    gen = torch.Generator().manual_seed(N + F)
    x = torch.randn((N, F), generator=gen).to(cuda)
    fused = ParamNet(F, RANGES, seed=3).to(cuda)
    ref = TorchParamNet(F, RANGES, seed=3).to(cuda)
    with torch.no_grad():  # non-zero biases, so their gradients and the bias paths are exercised
        b = torch.randn(param_count(F), generator=gen).to(cuda) * 0.1
        fused.flat.add_(b)
        ref.flat.add_(b)
    outs = fused(x)
    routs = ref(x)
    gs = [torch.randn(N, generator=gen).to(cuda) for _ in range(3)]
    for o, r in zip(outs, routs):
        assert o.shape == (N,)
        assert float(((o - r).abs() / r.abs().clamp_min(1e-6)).max()) <= 1e-5
    sum((o * g).sum() for o, g in zip(outs, gs)).backward()
    sum((o * g).sum() for o, g in zip(routs, gs)).backward()
    assert normrel(fused.flat.grad.cpu().numpy(), ref.flat.grad.cpu().numpy()) <= 1e-5


def test_fused_network_backward_is_deterministic(cuda):
    F, N = 10, 50000
    x = torch.randn((N, F), generator=torch.Generator().manual_seed(1)).to(cuda)
    net = ParamNet(F, RANGES).to(cuda)
    grads = []
    for _ in range(2):
        net.flat.grad = None
        n, q, p = net(x)
        (n.sum() + 2 * q.sum() + p.mean()).backward()
        grads.append(net.flat.grad.clone())
    assert torch.equal(grads[0], grads[1])
    assert np.isfinite(grads[0].cpu().numpy()).all()


def test_fused_network_rejects_misplaced_parameters(cuda):
    """The C ABI takes raw pointers: parameters left on the host, cast to fp64 or on another device must raise
    (a ValueError), not reach the kernel as fp32 device memory."""
    ranges = {"n": [0.015, 0.25], "q_spatial": [0.0, 1.0], "p_spatial": [1.0, 200.0]}
    x = torch.rand((1000, 10), device=cuda)
    net = ParamNet(10, ranges)
    with pytest.raises(ValueError):
        net(x)  # parameters still on the host
    net = net.to(cuda).double()
    with pytest.raises(ValueError):
        net(x)  # fp64 parameters
    net = net.float()
    outs = net(x)
    assert all(o.shape == (1000,) for o in outs)


# ---------------------------------------------------------------------------- against float64, block by block


@functools.lru_cache(maxsize=None)
def _reference(F, N, kind, table, only, row, ones):
    """The case's fp32 inputs (CPU) and its float64 result, computed once and left unchanged."""
    flat = tc.make_params(F)
    x = tc.make_inputs(kind, N, F)
    gouts = tc.make_gouts(N, only=only, row=row, ones=ones)
    outs, grad = tc.pnet_reference(F, tc.TABLES[table], flat, x, gouts)
    for a in (*outs, grad):
        a.setflags(write=False)
    return flat, x, gouts, outs, grad


def _on_device(cls, cuda, F, table, flat, x, loss_fn):
    ranges, log_space = tc.TABLES[table]
    net = cls(F, ranges, log_space).to(cuda)
    with torch.no_grad():
        net.flat.copy_(flat.to(cuda))
    outs = net(x.to(cuda))
    loss_fn(outs).backward()
    return [o.detach().cpu().numpy() for o in outs], net.flat.grad.cpu().numpy()


def check(cuda, F, N, kind="plain", table="default", only=None, row=None, ones=False, loss_fn=None):
    """R, T and K of one case; every output and gradient block of K within MARGIN of T's error against R.
    ``loss_fn`` replaces the weighted loss on the device (it must have the same gradient)."""
    flat, x, gouts, routs, rgrad = _reference(F, N, kind, table, only, row, ones)
    loss_fn = loss_fn or (lambda outs: tc.weighted_loss(outs, gouts))
    touts, tgrad = _on_device(TorchParamNet, cuda, F, table, flat, x, loss_fn)
    kouts, kgrad = _on_device(ParamNet, cuda, F, table, flat, x, loss_fn)
    figures = []
    for j, name in enumerate(("n", "q_spatial", "p_spatial")):
        assert kouts[j].shape == (N,) and kouts[j].dtype == np.float32
        figures.append((name, "maxrel", tc.out_error(touts[j], routs[j]), tc.out_error(kouts[j], routs[j])))
    et, ek = tc.block_errors(tgrad, rgrad, F), tc.block_errors(kgrad, rgrad, F)
    for name in tc.BLOCKS:
        figures.append(("d" + name, "normrel", et[name][0], ek[name][0]))
        figures.append(("d" + name, "maxabs", et[name][1], ek[name][1]))
    failed = []
    for name, metric, t, k in figures:
        bound = tc.bound(t, FIXED)
        print(f"pnet F={F} N={N} {kind} {table} only={only} row={row} ones={ones} {name} {metric}: "
              f"T {t:.3e} K {k:.3e} ratio {k / t if t > 0 else float('nan'):.2f}")
        if not k <= bound:
            failed.append((name, metric, t, k, bound))
    assert not failed, failed
    return figures


@pytest.mark.parametrize("F", [1, 2, 3, 4, 5, 8, 9, 11, 12])
def test_feature_widths(cuda, F):
    """The k-step boundaries of the padded first layer (``k < F``, ``f < F``, ``lq < F``), three tiles with two
    rows in the last."""
    check(cuda, F, 130)


@pytest.mark.parametrize("N,F", [(n, 10) for n in (1, 15, 16, 17, 63, 64, 65, 127, 128, 129)] + [(65, 3)])
def test_row_edges(cuda, N, F):
    """Either side of a 16-row fragment block and of a 64-row tile."""
    check(cuda, F, N)


def test_no_rows(cuda):
    F = 10
    net = ParamNet(F, RANGES).to(cuda)
    outs = net(torch.zeros((0, F), device=cuda))
    assert all(o.shape == (0,) and o.dtype == torch.float32 for o in outs)
    sum(o.sum() for o in outs).backward()
    assert net.flat.grad.shape == (param_count(F),)
    assert not net.flat.grad.cpu().numpy().any()


@pytest.mark.parametrize("N", ["cus+1", "2cus+1", 70001])
def test_persistent_loop(cuda, N):
    """64 C + 1 and 64 (2 C) + 1 rows (C compute units): exactly one workgroup takes a second tile in the backward
    and in the forward kernel.  70001 rows: several tiles per workgroup."""
    C = torch.cuda.get_device_properties(cuda).multi_processor_count
    check(cuda, 10, {"cus+1": 64 * C + 1, "2cus+1": 128 * C + 1}.get(N, N))


@pytest.mark.parametrize("table", ["linear", "all_log", "mock"])
def test_denormalisation_tables(cuda, table):
    """No log-space output; all three in log space with q_spatial's lower bound 0 (offset ln 1e-6); the mock
    configuration's ranges."""
    check(cuda, 10, 130, table=table)


@pytest.mark.parametrize("N", [130, 64])
@pytest.mark.parametrize("kind", ["plain", "saturating", "zeros", "constant_tile"])
def test_input_kinds(cuda, kind, N):
    """randn (the figures of DESIGN.md section 5 are this and the next case at N = 130); SiLU saturated on both
    sides and U within rounding of 0 and 1 (conditions: test_tail_cases.py); x = 0, whose dW1 is exactly zero; a
    tile of identical rows."""
    check(cuda, 10, N, kind=kind)


@pytest.mark.parametrize("only", [0, 1, 2])
def test_one_output_at_a_time(cuda, only):
    """The loss depends on one output: the other two output gradients are not dense random vectors but absent."""
    check(cuda, 10, 130, only=only)


def test_sum_of_one_output(cuda):
    """``n.sum()``: the output gradient arrives as a zero-stride expanded tensor."""
    check(cuda, 10, 130, only=0, ones=True, loss_fn=lambda outs: outs[0].sum())


@pytest.mark.parametrize("row", [0, 63, 64, 127, 128, 129])
def test_one_row_at_a_time(cuda, row):
    """The output gradient is non-zero on one row: a row mask or tile offset that dense gradients average away
    moves every block."""
    check(cuda, 10, 130, row=row)


def test_backward_is_deterministic_with_a_second_tile(cuda):
    F = 10
    N = 64 * torch.cuda.get_device_properties(cuda).multi_processor_count + 1
    x = tc.make_inputs("saturating", N, F).to(cuda)
    net = ParamNet(F, RANGES).to(cuda)
    with torch.no_grad():
        net.flat.copy_(tc.make_params(F).to(cuda))
    grads = []
    for _ in range(2):
        net.flat.grad = None
        n, q, p = net(x)
        (n.sum() + 2 * q.sum() + p.mean()).backward()
        grads.append(net.flat.grad.clone())
    assert torch.equal(grads[0], grads[1])
    assert np.isfinite(grads[0].cpu().numpy()).all()
