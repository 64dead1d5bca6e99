"""Shared by test_tail_cases.py, test_gpu_pnet.py and test_gpu_train.py: float64 CPU references of the C3 step tail
(the parameter network ``ddr_amd.pnet``, the daily L1 objective and clip + Adam of ``ddr_amd.train``), block-wise
error metrics of the flat parameter gradient, and input generators with fixed seeds."""

from __future__ import annotations

import math

import numpy as np
import torch

from conftest import PARAMS_DEFAULT, PARAMS_MOCK
from ddr_amd.pnet import HIDDEN, OUT, TorchParamNet, init_params, param_count

BLOCKS = ("w1", "b1", "w2", "b2", "w3", "b3", "w4", "b4")
RANGES = PARAMS_DEFAULT["parameter_ranges"]
# name -> (ranges, log_space): the denormalisation tables of the network tests.  "all_log" has q_spatial's lower
# bound 0, whose log-space offset is ln 1e-6
TABLES = {
    "default": (RANGES, ("p_spatial",)),
    "linear": (RANGES, ()),
    "all_log": (RANGES, ("n", "q_spatial", "p_spatial")),
    "mock": (PARAMS_MOCK["parameter_ranges"], ("p_spatial",)),
}
INPUT_KINDS = ("plain", "saturating", "zeros", "constant_tile")
TILE = 64  # rows per tile of csrc/pnet.hip

# The GPU tests bound the fused kernels' error against float64, err(K, R), by MARGIN times the error of the same
# operation in PyTorch fp32 ops on the device, err(T, R): one number for every case, output and block (chosen after
# measuring on the MI355X: DESIGN.md section 5).  Where err(T, R) is below one fp32 ulp (T is right to the last bit of
# the largest entry, as happens with one row, three entries or an identically zero block) the ratio says nothing and
# the bound is the file's fixed tolerance.
MARGIN = 8.0
TINY = 2.0 ** -23


def bound(t: float, fixed: float) -> float:
    return MARGIN * t if t >= TINY else fixed


def block_shapes(F: int):
    return [("w1", (HIDDEN, F)), ("b1", (HIDDEN,)), ("w2", (HIDDEN, HIDDEN)), ("b2", (HIDDEN,)),
            ("w3", (HIDDEN, HIDDEN)), ("b3", (HIDDEN,)), ("w4", (OUT, HIDDEN)), ("b4", (OUT,))]


def blocks(flat_or_grad, F: int) -> dict:
    """The eight named blocks of ``ddr_amd.pnet.views`` of a flat vector (NumPy views)."""
    a = np.asarray(flat_or_grad)
    assert a.shape == (param_count(F),), a.shape
    out, o = {}, 0
    for name, shp in block_shapes(F):
        k = math.prod(shp)
        out[name] = a[o:o + k].reshape(shp)
        o += k
    return out


def errors(a, ref) -> tuple[float, float]:
    """(normrel, maxabs) = (|a - ref|_2 / |ref|_2, max|a - ref| / max|ref|).  A reference that is identically zero
    must be met exactly: (0, 0) then, (inf, inf) otherwise."""
    a = np.asarray(a, np.float64)
    ref = np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    if a.size == 0:
        return 0.0, 0.0
    if not np.isfinite(a).all():
        return math.inf, math.inf
    if not ref.any():
        return (0.0, 0.0) if not a.any() else (math.inf, math.inf)
    d = a - ref
    return float(np.linalg.norm(d) / np.linalg.norm(ref)), float(np.abs(d).max() / np.abs(ref).max())


def block_errors(a, ref, F: int) -> dict:
    """name -> (normrel, maxabs) of each of the eight blocks.  One wrong element in one fragment lane shows in
    maxabs of its block even where the block's norm hides it."""
    ba, br = blocks(a, F), blocks(ref, F)
    return {name: errors(ba[name], br[name]) for name in BLOCKS}


def out_error(a, ref) -> float:
    """max-rel with the floor 1e-6 of tests/test_gpu_pnet.py."""
    a = np.asarray(a, np.float64)
    ref = np.asarray(ref, np.float64)
    if a.size == 0:
        return 0.0
    if not np.isfinite(a).all():
        return math.inf
    return float((np.abs(a - ref) / np.maximum(np.abs(ref), 1e-6)).max())


# ------------------------------------------------------------------------------------------- parameter network


def make_params(F: int, seed: int = 3) -> torch.Tensor:
    """The parameters of tests/test_gpu_pnet.py: ``init_params`` plus 0.1 randn everywhere, so the biases are
    non-zero (fp32, CPU)."""
    g = torch.Generator().manual_seed(1000 + F)
    return init_params(F, seed) + 0.1 * torch.randn(param_count(F), generator=g)


def make_inputs(kind: str, N: int, F: int) -> torch.Tensor:
    """(N, F) fp32 attributes.  ``plain``: randn.  ``saturating``: randn scaled so that hidden pre-activations
    pass +-20 and the sigmoid outputs come within 1e-4 of 0 and 1 (with ``make_params``; the conditions are
    asserted in test_tail_cases.py).  ``zeros``: x = 0.  ``constant_tile``: every row of one 64-row tile (the
    second where there is one) identical."""
    g = torch.Generator().manual_seed(7919 * F + N)
    x = torch.randn((N, F), generator=g)
    if kind == "plain":
        return x
    if kind == "saturating":
        return x * (12.0 * math.sqrt(10.0 / F))
    if kind == "zeros":
        return torch.zeros((N, F))
    if kind == "constant_tile":
        t = 1 if N > TILE else 0
        x[t * TILE:(t + 1) * TILE] = x[t * TILE].clone()
        return x
    raise ValueError(kind)


def make_gouts(N: int, seed: int = 0, only: int | None = None, row: int | None = None, ones: bool = False) -> list:
    """Three (N,) fp32 output gradients (randn; all 1 with ``ones``).  ``only``: the other two are ``None``.
    ``row``: non-zero on that row alone."""
    g = torch.Generator().manual_seed(31 * N + seed)
    gs = [torch.ones(N) if ones else torch.randn(N, generator=g) for _ in range(OUT)]
    if row is not None:
        keep = torch.zeros(N)
        keep[row] = 1.0
        gs = [t * keep for t in gs]
    if only is not None:
        gs = [t if j == only else None for j, t in enumerate(gs)]
    return gs


def weighted_loss(outs, gouts):
    """sum_j <out_j, g_j> over the outputs that have a gradient: its backward hands the network exactly ``gouts``."""
    return sum((o * g.to(device=o.device, dtype=o.dtype)).sum() for o, g in zip(outs, gouts) if g is not None)


def _torch_net(F: int, table_args, flat) -> TorchParamNet:
    ranges, log_space = table_args
    net = TorchParamNet(F, ranges, log_space)
    with torch.no_grad():
        net.flat.copy_(torch.as_tensor(flat, dtype=torch.float32))
    return net


def pnet_reference(F: int, table_args, flat, x, gouts):
    """``TorchParamNet`` in float64 on the CPU through autograd: the three outputs (N,) and the gradient of
    ``weighted_loss`` with respect to the flat parameters, as float64 NumPy arrays."""
    net = _torch_net(F, table_args, flat).double()
    outs = net(torch.as_tensor(x).double())
    if any(g is not None for g in gouts) and x.shape[0] > 0:
        weighted_loss(outs, gouts).backward()
        grad = net.flat.grad.numpy().copy()
    else:
        grad = np.zeros(param_count(F))
    return [o.detach().numpy().copy() for o in outs], grad


def pnet_internals(F: int, flat, x):
    """The float64 hidden pre-activations Z1..Z3 (3, N, 128) and sigmoid outputs U (N, 3)."""
    b = blocks(np.asarray(flat, np.float64), F)
    h = np.asarray(x, np.float64)
    zs = []
    for l in ("1", "2", "3"):
        z = h @ b["w" + l].T + b["b" + l]
        zs.append(z)
        h = z / (1.0 + np.exp(-z))
    return np.stack(zs), 1.0 / (1.0 + np.exp(-(h @ b["w4"].T + b["b4"])))


# ------------------------------------------------------------------------------------------------- clip + Adam


def adam_reference(p0, grads, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_norm=1.0):
    """``clip_grad_norm_(max_norm)`` (coef = min(max_norm / (norm + 1e-6), 1); none for max_norm <= 0), then textbook
    Adam (bias-corrected, no weight decay, no amsgrad), once per entry of ``grads``, in float64.
    Returns (params, m, v, [norm of every step])."""
    p = np.array(p0, np.float64)
    m = np.zeros_like(p)
    v = np.zeros_like(p)
    b1, b2 = betas
    norms = []
    for t, g in enumerate(grads, 1):
        g = np.asarray(g, np.float64)
        norm = float(np.sqrt((g * g).sum()))
        norms.append(norm)
        if max_norm > 0:
            g = g * min(max_norm / (norm + 1e-6), 1.0)
        m = b1 * m + (1.0 - b1) * g
        v = b2 * v + (1.0 - b2) * g * g
        p = p - lr * (m / (1.0 - b1 ** t)) / (np.sqrt(v / (1.0 - b2 ** t)) + eps)
    return p, m, v, norms


def torch_adam(p0: torch.Tensor, grads, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_norm=1.0):
    """``torch.optim.Adam`` + ``torch.nn.utils.clip_grad_norm_`` in ``p0``'s dtype on its device.
    Returns (params, m, v, [norm of every step]) as float64 NumPy."""
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=eps)
    norms = []
    for g in grads:
        p.grad = g.to(device=p.device, dtype=p.dtype).clone()
        if max_norm > 0:
            norms.append(float(torch.nn.utils.clip_grad_norm_([p], max_norm=max_norm)))
        else:
            norms.append(float(torch.linalg.vector_norm(p.grad)))
        opt.step()
    st = opt.state[p]
    f = lambda t: t.detach().double().cpu().numpy()  # noqa: E731
    return f(p), f(st["exp_avg"]), f(st["exp_avg_sq"]), norms


def adam_grads(n: int, steps: int, scale: float, seed: int = 0) -> list:
    """``steps`` fresh fp32 randn gradients of length n times ``scale`` (CPU)."""
    g = torch.Generator().manual_seed(104729 * seed + n)
    return [torch.randn(n, generator=g) * scale for _ in range(steps)]


# ------------------------------------------------------------------------------------------------- daily L1

L1_SHAPES = [(1, 1, 0), (1, 7, 6), (3, 5, 0), (4, 256, 1), (1023, 1, 0), (1025, 1, 0), (256, 89, 88), (1000, 365, 30)]


def l1_inputs(G: int, D: int, warmup: int):
    """fp32 (G, D) daily and obs with, after the warm-up, at least one exactly zero difference and (where more than
    one element is left) both signs; one zero difference inside the warm-up too where there is one."""
    g = torch.Generator().manual_seed(G * 1009 + D * 17 + warmup)
    daily = torch.rand((G, D), generator=g)
    obs = torch.rand((G, D), generator=g)
    live = [(i, d) for i in range(min(G, 3)) for d in range(warmup, min(D, warmup + 3))]
    obs[live[0]] = daily[live[0]]
    if len(live) > 1:
        obs[live[1]] = daily[live[1]] + 0.25
    if len(live) > 2:
        obs[live[2]] = daily[live[2]] - 0.25
    if warmup > 0:
        obs[0, 0] = daily[0, 0]
    return daily, obs


def l1_reference(daily, obs, warmup: int, inv_count: float | None = None):
    """float64: loss = inv_count sum |daily - obs| after the warm-up (the mean's 1 / (G (D - warmup)) by default) and
    its gradient sign(diff) inv_count, 0 before the warm-up."""
    daily = np.asarray(daily, np.float64)
    obs = np.asarray(obs, np.float64)
    G, D = daily.shape
    if inv_count is None:
        inv_count = 1.0 / (G * (D - warmup))
    diff = daily - obs
    diff[:, :warmup] = 0.0
    return float(np.abs(diff).sum() * inv_count), np.sign(diff) * inv_count
