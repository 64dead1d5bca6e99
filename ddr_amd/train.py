"""The tail of the C3 training step on the device in three launches (``csrc/train.hip``).

The reference's loop (``scripts/train.py:91-100``) ends each mini-batch with ``l1_loss`` over the gauges'
daily series after the warm-up, ``loss.backward()``, ``clip_grad_norm_(max_norm=1.0)`` and ``optimizer.step()``
(Adam).  In PyTorch ops that is ~15 small launches per step (slice, subtract, abs, sum, scale and their
backward; the norm, the clip factor, the scaling; Adam's moment updates).  Here:

* :func:`daily_l1_loss` -- the objective and its gradient in one pass (``ddr_daily_l1_f32``); the backward is
  one multiply by the incoming scalar;
* :func:`daily_objective` -- the masked objective family (``ddr_daily_objective_f32``, ``csrc/objective.hip``): L1,
  MSE, 1 - NSE and 1 - KGE with a NaN observation as a missing day and a dropped gauge as a mask, so a step on real
  observations needs no boolean indexing, no host sync and can be captured;
* :class:`ClipAdam` -- clip + Adam over one flat parameter vector (``ddr_clip_adam_f32``), e.g.
  :class:`ddr_amd.pnet.ParamNet`'s ``flat``.

Both are deterministic (fixed slices and reduction order) and run on the HIP device only.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import torch

from . import _lib


class _DailyL1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, daily, obs, warmup, inv_count):
        G, D = daily.shape
        loss = torch.empty((), device=daily.device, dtype=torch.float32)
        grad = torch.empty_like(daily) if ctx.needs_input_grad[0] else None
        _lib.check(_lib.load().ddr_daily_l1_f32(G, D, int(warmup), daily.data_ptr(), obs.data_ptr(), C.c_float(inv_count),
                                                loss.data_ptr(), grad.data_ptr() if grad is not None else None,
                                                _lib.stream_ptr(daily.device)))
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None, None, None


def daily_l1_loss(daily: torch.Tensor, obs: torch.Tensor, warmup: int, inv_count: float | None = None) -> torch.Tensor:
    """``inv_count * sum |daily[:, warmup:] - obs[:, warmup:]|`` (G, D) -> scalar; ``inv_count`` defaults to the
    mean's 1 / (G (D - warmup)) -- ``torch.nn.functional.l1_loss(daily[:, warmup:], obs[:, warmup:])``."""
    if not daily.is_cuda:
        raise RuntimeError("daily_l1_loss runs on the HIP device only (no CPU fallback)")
    if daily.dim() != 2 or obs.shape != daily.shape:
        raise ValueError("daily and obs must be the same (G, D) shape")
    G, D = daily.shape
    if not 0 <= warmup < D:
        raise ValueError("warmup must be in [0, D)")
    if inv_count is None:
        inv_count = 1.0 / (G * (D - warmup))
    daily = daily.to(torch.float32).contiguous()
    obs = obs.to(device=daily.device, dtype=torch.float32).contiguous()
    return _DailyL1.apply(daily, obs, warmup, float(inv_count))

#: the objectives of :func:`daily_objective` (``DDR_OBJECTIVE_*`` order in ``include/ddr_mc.h``)
OBJECTIVE_KINDS = _lib.OBJECTIVE_KINDS
MAX_DAYS = 8192


@dataclass
class ObjectiveTerms:
    """Per-gauge values of one :func:`daily_objective` call, (G,) fp64 device tensors: ``term`` (NaN where the gauge
    is not used), ``days`` n_g, the counted days, and ``used`` (0 / 1)."""

    term: torch.Tensor
    days: torch.Tensor
    used: torch.Tensor


class _DailyObjective(torch.autograd.Function):
    @staticmethod
    def forward(ctx, daily, obs, warmup, kind, drop, weight, eps, count, table):
        G, D = daily.shape
        with torch.cuda.device(daily.device):
            # (G == 0 is a no-op of the library: the loss of nothing is 0)
            loss = (torch.empty if G else torch.zeros)((), device=daily.device, dtype=torch.float32)
            grad = torch.empty((G, D), device=daily.device, dtype=torch.float32) if ctx.needs_input_grad[0] else None
            lib = _lib.load()
            work = torch.empty(int(lib.ddr_daily_objective_work_bytes(G)) // 8, device=daily.device, dtype=torch.float64)
            desc = _lib.ObjectiveDesc(kind, 0, G, D, int(warmup), float(eps))
            by_value = 0.0 if count is None or isinstance(count, torch.Tensor) else float(count)
            _lib.check(lib.ddr_daily_objective_f32(
                C.byref(desc), daily.data_ptr(), daily.stride(0), obs.data_ptr(), obs.stride(0), _lib.ptr(drop),
                _lib.ptr(weight), C.c_double(by_value), _lib.ptr(count) if isinstance(count, torch.Tensor) else None,
                loss.data_ptr(), _lib.ptr(grad), _lib.ptr(table), work.data_ptr(), _lib.stream_ptr(daily.device)))
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return (grad * g,) + (None,) * 8


def daily_objective(daily: torch.Tensor, obs: torch.Tensor, warmup: int, kind: str = "l1", *,
                    drop: torch.Tensor | None = None, weight: torch.Tensor | None = None, eps: float = 0.0,
                    count: float | torch.Tensor | None = None, terms: bool = False):
    """A masked training objective over (G, D) fp32 daily series -> scalar loss, differentiable w.r.t. ``daily``.

    A NaN in ``obs`` is a missing day; ``drop`` (G,) bool removes whole gauges -- ``ObservationStore.window``'s
    ``has_nan`` reproduces the reference's filter (``scripts/train.py:84-92``) without changing a shape or waiting
    for the device.  Over the counted days of gauge g (day >= ``warmup``, observed, not dropped; n_g of them):

    * ``"l1"`` / ``"mse"``: the mean of abs(p - o) / (p - o)^2 over every counted day of every gauge (weighted by
      ``weight[g]``); with ``drop=has_nan``, ``"l1"`` equals ``l1_loss(daily[keep][:, warmup:], obs[keep][:, warmup:])``;
    * ``"nse"``: the mean over gauges with n_g >= 2 of sum (p - o)^2 / (n_g (std_o + eps)^2) -- 1 - NSE at eps = 0
      (a constant target is skipped unless eps > 0);
    * ``"kge"``: the mean over gauges of 1 - KGE (``ddr.validation.metrics``' r, alpha, beta); gauges with fewer than
      two days, a constant or zero-mean target or a constant prediction are skipped.

    ``count`` overrides the normaliser (ranks that all-reduce their counts): a float goes in by value, a fp32 device
    scalar by pointer, so a captured step can update it in place.  When nothing is used the loss and the gradient are
    0.  ``terms=True`` also returns :class:`ObjectiveTerms`.  Rows of any stride are read in place; a tensor whose
    innermost stride is not 1 is made contiguous.  Deterministic; at most three launches; HIP device only."""
    if not isinstance(daily, torch.Tensor) or not isinstance(obs, torch.Tensor):
        raise TypeError("daily_objective takes torch tensors")
    if kind not in OBJECTIVE_KINDS:
        raise ValueError(f"kind must be one of {OBJECTIVE_KINDS}, not {kind!r}")
    if daily.dtype != torch.float32 or obs.dtype != torch.float32:
        raise ValueError("daily and obs must be float32")
    if daily.dim() != 2 or obs.shape != daily.shape:
        raise ValueError("daily and obs must be the same (G, D) shape")
    G, D = daily.shape
    if not 1 <= D <= MAX_DAYS:
        raise ValueError(f"daily_objective takes 1 to {MAX_DAYS} days, not {D}")
    if int(warmup) != warmup or not 0 <= warmup < D:
        raise ValueError("warmup must be an integer in [0, D)")
    if not eps >= 0.0:
        raise ValueError("eps must be >= 0")
    if drop is not None and (drop.dtype != torch.bool or drop.shape != (G,)):
        raise ValueError("drop must be a (G,) bool tensor")
    if weight is not None and (weight.dtype != torch.float32 or weight.shape != (G,)):
        raise ValueError("weight must be a (G,) float32 tensor")
    if isinstance(count, torch.Tensor):
        if count.dtype != torch.float32 or count.numel() != 1:
            raise ValueError("count as a tensor must be a float32 scalar")
    elif count is not None and not float(count) > 0.0:
        raise ValueError("count must be > 0")
    if not daily.is_cuda:
        raise RuntimeError("daily_objective runs on the HIP device only (no CPU fallback)")
    for name, t in (("obs", obs), ("drop", drop), ("weight", weight), ("count", count)):
        if isinstance(t, torch.Tensor) and t.device != daily.device:
            raise ValueError(f"{name} must be on daily's device")
    if daily.stride(1) != 1:
        daily = daily.contiguous()
    if obs.stride(1) != 1:
        obs = obs.contiguous()
    drop = drop.contiguous() if drop is not None else None
    weight = weight.contiguous() if weight is not None else None
    table = torch.empty((3, G), device=daily.device, dtype=torch.float64) if terms else None
    loss = _DailyObjective.apply(daily, obs, int(warmup), OBJECTIVE_KINDS.index(kind), drop, weight, float(eps), count,
                                 table)
    if not terms:
        return loss
    return loss, ObjectiveTerms(table[0], table[1], table[2])


class ClipAdam:
    """``clip_grad_norm_(max_norm)`` then ``torch.optim.Adam(lr, betas, eps)`` (no weight decay) on one flat
    fp32 parameter tensor, in two launches per step (64 workgroups).  ``max_norm`` <= 0 disables clipping.  ``last_norm`` holds the
    gradient norm of the last step (a device scalar, clip_grad_norm_'s return value).

    Unlike ``torch.nn.utils.clip_grad_norm_``, the clip is applied inside the update only: ``param.grad`` keeps
    the unclipped gradient after :meth:`step` (code that reads or accumulates ``.grad`` afterwards sees the raw
    gradient, not the reference loop's clipped one, ``scripts/train.py:99-100``)."""

    def __init__(self, param: torch.Tensor, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 max_norm: float = 1.0):
        if not param.is_cuda or param.dtype != torch.float32 or not param.is_contiguous():
            raise ValueError("ClipAdam takes one contiguous fp32 HIP parameter tensor")
        self.param = param
        self.lr, self.betas, self.eps, self.max_norm = float(lr), tuple(map(float, betas)), float(eps), float(max_norm)
        self.m = torch.zeros_like(param)
        self.v = torch.zeros_like(param)
        self.last_norm = torch.zeros((), device=param.device, dtype=torch.float32)
        self.work = torch.empty(int(_lib.load().ddr_clip_adam_work_bytes()), device=param.device, dtype=torch.uint8)
        # the step counter lives on the device (as torch's capturable Adam): a captured step replays correctly
        self.step_count = torch.zeros((), device=param.device, dtype=torch.float32)

    def zero_grad(self, set_to_none: bool = True) -> None:
        if set_to_none:
            self.param.grad = None
        elif self.param.grad is not None:
            self.param.grad.zero_()

    @torch.no_grad()
    def step(self) -> None:
        g = self.param.grad
        if g is None:
            return
        g = g.contiguous()
        b1, b2 = self.betas
        _lib.check(_lib.load().ddr_clip_adam_f32(self.param.numel(), self.param.data_ptr(), g.data_ptr(),
                                                 self.m.data_ptr(), self.v.data_ptr(), C.c_float(self.lr), C.c_double(b1),
                                                 C.c_double(b2), C.c_float(self.eps), self.step_count.data_ptr(),
                                                 C.c_float(self.max_norm), self.last_norm.data_ptr(),
                                                 self.work.data_ptr(), _lib.stream_ptr(self.param.device)))
