"""The linear routing's adjoint on the CPU: the NumPy statement of the reverse sweep (tests/linear_adjoint_cases.py)
against torch's fp64 autograd of an independent forward, and ``ddr_amd.routing.muskingum_coefficient_gradients``, the
closed-form coefficient derivatives that sweep combines its parameter sums with (nothing here touches a device; the
package has no device adjoint yet, this is the reference one will be held to).

The bar of the fp64 comparison is ``1000 (F S + max_depth) 2^-53`` of the reference's largest entry, per tensor:
term count times unit roundoff, three decades for the cancelling combination of gk and gx (the three coefficient
derivatives sum to zero).  |C| <= 1 over K_RANGE x X_RANGE at dt = 900, so the recurrence does not amplify."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import linear_adjoint_cases as AC
import linear_cases as LC
import time_axis_cases as TA
from ddr_amd.network import Network
from ddr_amd.routing import muskingum_coefficient_gradients

DT = 900.0
U64 = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def tree():
    net = TA.network("S")
    return net, LC.Topology.of_coo(net.n, net.rows, net.cols)


@functools.lru_cache(maxsize=None)
def sandbox():
    d = LC.sandbox()
    net = Network.build(d["ids"], d["next_down"])
    return d, net, LC.Topology.of_coo(net.n, net.rows, net.cols)


def start(kind, n):
    return {"zero": None, "steady": "steady", "array": np.random.default_rng(77).uniform(0.0, 9.0, n)}[kind]


def compare(topo, k, x, dt, S, qext, q0, output, what):
    n, F = topo.n, qext.shape[0]
    gout, glast = AC.random_seeds(n, F, 5, np.float64)
    got = AC.adjoint(topo, k, x, dt, S, qext, q0=q0, output=output, gout=gout, glast=glast, dtype=np.float64)
    ref = AC.autograd_reference(topo, k, x, dt, S, qext, q0, output, gout, glast)
    bar = 1000.0 * (F * S + len(topo.levels)) * U64
    for name, r in ref.items():
        err = float(np.max(np.abs(got[name] - r)) / np.max(np.abs(r)))
        print(f"{what} {output} {name}: {err:.3e} (bar {bar:.3e})")
        assert err <= bar, (what, output, name, err, bar)
    assert set(ref) >= {"gqext", "gk", "gx"}


@pytest.mark.parametrize("output", ["mean", "end"])
@pytest.mark.parametrize("q0kind", ["zero", "array", "steady"])
def test_sandbox_against_autograd(output, q0kind):
    d, net, topo = sandbox()
    qext = net.align(d["qext"], axis=1).astype(np.float64)
    q0 = net.align(d["qinit"]).astype(np.float64) if q0kind == "array" else start(q0kind, net.n)
    compare(topo, float(d["k"]), float(d["x"]), float(d["dt"]), int(d["substeps"]), qext, q0, output, f"sandbox {q0kind}")


@pytest.mark.parametrize("output", ["mean", "end"])
@pytest.mark.parametrize("q0kind", ["zero", "array", "steady"])
@pytest.mark.parametrize("F,S", [(5, 7), (17, 3)])
def test_tree_against_autograd(F, S, q0kind, output):
    net, topo = tree()
    k, x = LC.parameters(net.n, 1, np.float64)
    qext = LC.random_forcing(net.n, F, 2, np.float64)
    compare(topo, k, x, DT, S, qext, start(q0kind, net.n), output, f"S ({F}, {S}) {q0kind}")


def test_flow_scale_and_valid_against_autograd():
    net, topo = tree()
    F, S = 6, 4
    k, x = LC.parameters(net.n, 1, np.float64)
    qext = LC.random_forcing(net.n, F, 2, np.float64)
    rng = np.random.default_rng(78)
    valid = np.ones(net.n, np.uint8)
    valid[rng.choice(net.n, 7, replace=False)] = 0
    fs = rng.uniform(0.5, 1.5, net.n)
    gout, glast = AC.random_seeds(net.n, F, 5, np.float64)
    got = AC.adjoint(topo, k, x, DT, S, qext, output="mean", gout=gout, glast=glast, flow_scale=fs, valid=valid)
    ref = AC.autograd_reference(topo, k, x, DT, S, qext, None, "mean", gout, glast, flow_scale=fs, valid=valid)
    bar = 1000.0 * (F * S + len(topo.levels)) * U64
    for name in ("gqext", "gk", "gx", "gflow_scale"):
        err = float(np.max(np.abs(got[name] - ref[name])) / np.max(np.abs(ref[name])))
        print(f"scaled {name}: {err:.3e} (bar {bar:.3e})")
        assert err <= bar, (name, err, bar)
    assert np.all(got["gqext"][:, valid == 0] == 0) and np.all(ref["gqext"][:, valid == 0] == 0)


def test_gauge_seeds_against_autograd():
    net, topo = tree()
    F, S = 6, 4
    gauges = TA.gauge_sets(net.n, 3)
    k, x = LC.parameters(net.n, 1, np.float64)
    qext = LC.random_forcing(net.n, F, 2, np.float64)
    grows = np.random.default_rng(9).uniform(-1.0, 1.0, (len(gauges), F))
    seeds = AC.gauge_seeds(grows, gauges, net.n, F, np.float64)
    got = AC.adjoint(topo, k, x, DT, S, qext, gout=seeds)
    # the reference differentiates the gauge rows themselves
    kt, xt, qt = (torch.tensor(v, requires_grad=True) for v in (k, x, qext))
    mean, _, _ = AC.torch_route(AC.adjacency(topo), kt, xt, DT, S, qt)
    rows = torch.stack([mean[torch.as_tensor(np.asarray(i) % net.n)].sum(0) for i in gauges])
    ref = torch.autograd.grad((rows * torch.as_tensor(grows)).sum(), (qt, kt, xt))
    bar = 1000.0 * (F * S + len(topo.levels)) * U64
    for name, r in zip(("gqext", "gk", "gx"), ref):
        err = float(np.max(np.abs(got[name] - r.numpy())) / np.max(np.abs(r.numpy())))
        assert err <= bar, (name, err, bar)


def autograd_derivatives(k, x, dt):
    kt, xt = torch.tensor(k, requires_grad=True), torch.tensor(x, requires_grad=True)
    h = dt / 2
    den = kt * (1 - xt) + h
    cs = ((h - kt * xt) / den, (h + kt * xt) / den, (kt * (1 - xt) - h) / den)
    pairs = [torch.autograd.grad(c.sum(), (kt, xt), retain_graph=True) for c in cs]
    return [p[0].numpy() for p in pairs], [p[1].numpy() for p in pairs]


def test_coefficient_gradients_against_autograd():
    """``muskingum_coefficient_gradients`` against autograd of the coefficients in fp64: a quotient of a few rounded
    operations each, 16 units of roundoff of the largest entry."""
    k, x = LC.parameters(257, 3, np.float64)
    rk, rx = autograd_derivatives(k, x, DT)
    for got in (muskingum_coefficient_gradients(k, x, DT),
                tuple(tuple(t.numpy() for t in s) for s in muskingum_coefficient_gradients(
                    torch.from_numpy(k), torch.from_numpy(x), DT))):
        dk, dx = got
        for j in range(3):
            for g_, ref in ((dk[j], rk[j]), (dx[j], rx[j])):
                assert g_.dtype == np.float64 and g_.shape == ref.shape
                assert np.max(np.abs(g_ - ref) / np.abs(ref).max()) <= 16 * U64
        # each set sums to zero: C1 + C2 + C3 = 1
        assert np.max(np.abs(sum(dk)) / np.abs(dk[2])) <= 8 * U64 and np.max(np.abs(sum(dx)) / np.abs(dx[1])) <= 8 * U64


def test_coefficient_gradients_dtypes_and_scalars():
    """fp32 parameters: fp64 results, of the fp32 values and of dt / 2 as the routing rounds it; a scalar x and
    ``linear_storage``'s x = 0 broadcast; tensors and arrays agree bit for bit."""
    k32, x32 = LC.parameters(64, 3, np.float32)
    dt = 900.1  # not a float32
    dk, dx = muskingum_coefficient_gradients(k32, x32, dt)
    assert all(v.dtype == np.float64 for v in dk + dx)
    h = np.float64(np.float32(dt) / np.float32(2))
    kd, xd = k32.astype(np.float64), x32.astype(np.float64)
    d2 = (kd * (1.0 - xd) + h) ** 2
    assert np.array_equal(dk[0], -h / d2) and np.array_equal(dx[0], -(kd * kd) / d2)
    tk, tx = muskingum_coefficient_gradients(torch.from_numpy(k32), torch.from_numpy(x32), dt)
    for a, b in zip(dk + dx, tk + tx):
        assert b.dtype == torch.float64 and np.array_equal(a, b.numpy())
    sk, sx = muskingum_coefficient_gradients(k32, 0.0, dt)  # linear_storage
    assert np.array_equal(sk[1], sk[0]) and sx[0].shape == k32.shape  # x = 0: dC2/dk = h (2 x - 1) / den^2 = dC1/dk
    lk, _ = muskingum_coefficient_gradients([9000.0, 9000.0], 0.25, 900.0)  # the Sandbox's parameters, plain lists
    assert lk[0].dtype == np.float64 and np.array_equal(lk[0], np.full(2, -450.0 / 7200.0 ** 2))


def test_fp32_model_near_fp64():
    net, topo = tree()
    F, S = 17, 3
    k, x = LC.parameters(net.n, 1, np.float32)
    qext = LC.random_forcing(net.n, F, 2, np.float32)
    gout, glast = AC.random_seeds(net.n, F, 5, np.float32)
    a32 = AC.adjoint(topo, k, x, DT, S, qext, gout=gout, glast=glast, dtype=np.float32)
    a64 = AC.adjoint(topo, k, x, DT, S, qext, gout=gout, glast=glast, dtype=np.float64)
    for name in ("gqext", "gk", "gx"):
        err = float(np.max(np.abs(a32[name] - a64[name])) / np.max(np.abs(a64[name])))
        print(f"fp32 model vs fp64 model, {name}: {err:.3e}")
        assert a32[name].dtype == np.float32 and err <= 1e-4
