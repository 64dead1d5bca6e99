"""``ddr_amd.routing.muskingum_coefficient_gradients`` on device tensors: the bits of the host evaluation (fp64
products, sums and quotients, which the device rounds as the host does), and the parameters of a routed case."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import linear_cases as LC
from ddr_amd.routing import muskingum_coefficient_gradients, muskingum_coefficients

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("npd", [np.float32, np.float64])
def test_device_tensors_give_the_host_bits(cuda, npd):
    k, x = LC.parameters(1031, 1, npd)
    dt = 900.1
    want = muskingum_coefficient_gradients(k, x, dt)
    got = muskingum_coefficient_gradients(torch.from_numpy(k).to(cuda), torch.from_numpy(x).to(cuda), dt)
    for ws, gs in zip(want, got):
        for w, g in zip(ws, gs):
            assert g.is_cuda and g.dtype == torch.float64
            assert np.array_equal(w.view(np.uint64), g.cpu().numpy().view(np.uint64))


def test_chain_rule_through_the_coefficients(cuda):
    """dL/dk and dL/dx of a loss on the device coefficients, by the closed forms, against autograd of
    ``muskingum_coefficients`` on the same device tensors: 16 units of fp64 roundoff of the largest term."""
    kn, xn = LC.parameters(513, 2, np.float64)
    k = torch.from_numpy(kn).to(cuda).requires_grad_(True)
    x = torch.from_numpy(xn).to(cuda).requires_grad_(True)
    w = [torch.from_numpy(np.random.default_rng(s).uniform(-1.0, 1.0, 513)).to(cuda) for s in (1, 2, 3)]
    c = muskingum_coefficients(k, x, 900.0)
    gk, gx = torch.autograd.grad(sum((wi * ci).sum() for wi, ci in zip(w, c)), (k, x))
    dk, dx = muskingum_coefficient_gradients(k.detach(), x.detach(), 900.0)
    for ref, d in ((gk, dk), (gx, dx)):
        got = (w[0] * d[0] + w[1] * d[1]) + w[2] * d[2]
        terms = sum((wi * di).abs() for wi, di in zip(w, d))
        assert bool(((got - ref).abs() <= 16 * 2.0 ** -53 * terms.max()).all())
