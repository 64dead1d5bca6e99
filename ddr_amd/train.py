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

* :func:`step_summary` -- the step's log record (``scripts/train.py:110-132``): the means and medians over gauges of
  NSE, RMSE and KGE and the min / median / max of the routing parameters, from :func:`ddr_amd.stats.summarize` calls
  alone, read back with one small copy when a log line is due.

All are deterministic (fixed slices and reduction order) and run on the HIP device only.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import torch

from . import _lib
from .stats import SUMMARY_COLUMNS, summarize
from .validation.metrics import METRIC_NAMES


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


_RULE = "-" * 40
_COL = {name: k for k, name in enumerate(SUMMARY_COLUMNS + ("median",))}
#: the rows of :attr:`StepSummary.record` before the parameters' rows
STEP_METRICS = ("nse", "rmse", "kge")


@dataclass
class StepSummary:
    """The log record of one step.  ``record`` is one (3 + P, 6) fp64 device tensor: rows ``nse, rmse, kge`` (over the
    gauges; NSE without its NaN and +-inf entries) and one row per parameter in ``names`` order, columns ``count, min,
    max, mean, std, median`` as :func:`ddr_amd.stats.summarize` wrote them.  ``sizes`` holds the parameters' lengths
    (host integers: a NaN count is the length minus the count)."""

    record: torch.Tensor
    names: tuple
    sizes: tuple

    def read(self) -> dict:
        """The single device-to-host copy.  Returns ``nse_mean, nse_median, rmse_mean, rmse_median, kge_mean,
        kge_median`` and then, per parameter, ``{name}_min, {name}_median, {name}_max, {name}_nan_count``, in
        this order (floats; the counts are ints)."""
        return self.decode(self.record.cpu())

    def decode(self, host) -> dict:
        """:meth:`read`'s dict from a host copy of ``record`` (a (3 + P, 6) tensor, array or nested list)."""
        rows = [[float(v) for v in row] for row in (host.tolist() if hasattr(host, "tolist") else host)]
        if len(rows) != len(STEP_METRICS) + len(self.names) or any(len(r) != len(_COL) for r in rows):
            raise ValueError(f"the record must be ({len(STEP_METRICS) + len(self.names)}, {len(_COL)})")
        out = {}
        for k, m in enumerate(STEP_METRICS):
            out[f"{m}_mean"] = rows[k][_COL["mean"]]
            out[f"{m}_median"] = rows[k][_COL["median"]]
        for k, (name, size) in enumerate(zip(self.names, self.sizes)):
            row = rows[len(STEP_METRICS) + k]
            out[f"{name}_min"] = row[_COL["min"]]
            out[f"{name}_median"] = row[_COL["median"]]
            out[f"{name}_max"] = row[_COL["max"]]
            out[f"{name}_nan_count"] = int(size) - int(row[_COL["count"]])
        return out

    def lines(self, epoch: int | None = None, mini_batch: int | None = None, values: dict | None = None) -> list:
        """The reference's log lines for this step: ``utils.log_metrics``' table (``validation/utils.py:104-113``) and
        one ``"{name}: min=..., median=..., max=..."`` line per parameter (``scripts/train.py:128-132``), with the
        same format strings; the caller logs them.  ``values`` is :meth:`read`'s dict (read now when not given).
        A parameter that holds NaN gets `` (nan_count=k)`` appended: its NaN are counted, not propagated."""
        v = self.read() if values is None else values
        out = []
        if epoch is not None and mini_batch is not None:
            out += [_RULE, f"Epoch: {epoch:<9} | Mini Batch: {mini_batch:<8} "]
        out += [_RULE, f"{'Metric':<10} | {'Mean':>12} | {'Median':>12}", _RULE]
        for m in STEP_METRICS:
            out.append(f"{m.upper():<10} | {v[f'{m}_mean']:12.4f} | {v[f'{m}_median']:12.4f}")
        out.append(_RULE)
        for name in self.names:
            line = (f"{name}: min={v[f'{name}_min']:.6f}, median={v[f'{name}_median']:.6f}, "
                    f"max={v[f'{name}_max']:.6f}")
            if v[f"{name}_nan_count"]:
                line += f" (nan_count={v[f'{name}_nan_count']})"
            out.append(line)
        return out


def step_summary(metric_values: torch.Tensor, params, *, out: torch.Tensor | None = None) -> StepSummary:
    """The step's log record on the device, replacing ``scripts/train.py:110-132``'s host work (``nanmean`` /
    ``nanmedian`` over gauges, and per parameter a ``.cpu()`` with ``min / median / max``).

    ``metric_values`` is :func:`ddr_amd.validation.metrics_device`'s (18, G) fp64 tensor; ``params`` an ordered
    mapping of name -> (N,) fp32 tensor (``routing_model.n / q_spatial / p_spatial``).  Only
    :func:`~ddr_amd.stats.summarize` calls are issued, each writing its rows of the record in place: the NSE row
    with ``skip_inf`` (the reference drops its NaN and +-inf entries), the RMSE and KGE rows as one strided view,
    and one call per parameter with the ``lower`` median (``torch.median``'s element).  No host sync: a captured
    step can hold it, with ``out`` a fixed contiguous (3 + P, 6) fp64 tensor.

    One deviation: the reference's ``torch.min / median / max`` propagate a NaN in a parameter; here NaN are left
    out and counted (``{name}_nan_count``)."""
    if not isinstance(metric_values, torch.Tensor):
        raise TypeError("step_summary takes metrics_device's tensor")
    if metric_values.dtype != torch.float64 or metric_values.dim() != 2 or metric_values.shape[0] != len(METRIC_NAMES):
        raise ValueError(f"metric_values must be the ({len(METRIC_NAMES)}, G) float64 tensor of metrics_device")
    if not hasattr(params, "items"):
        raise ValueError("params must be a mapping of name -> (N,) float32 tensor")
    items = [(str(k), v) for k, v in params.items()]
    for name, t in items:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 1:
            raise ValueError(f"parameter {name!r} must be a (N,) float32 tensor")
        if t.device != metric_values.device:
            raise ValueError(f"parameter {name!r} must be on metric_values' device")
    rows = len(STEP_METRICS) + len(items)
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float64
                            or out.shape != (rows, len(_COL)) or not out.is_contiguous()
                            or out.device != metric_values.device):
        raise ValueError(f"out must be a contiguous ({rows}, {len(_COL)}) float64 tensor on metric_values' device")
    if not metric_values.is_cuda:
        raise RuntimeError("step_summary runs on the HIP device only (no CPU fallback)")
    mv = metric_values.detach()
    if mv.shape[1] > 1 and mv.stride(1) != 1:
        mv = mv.contiguous()
    i_nse, i_rmse, i_kge = (METRIC_NAMES.index(m) for m in STEP_METRICS)
    with torch.cuda.device(mv.device):
        rec = out if out is not None else torch.empty((rows, len(_COL)), device=mv.device, dtype=torch.float64)
        summarize(mv[i_nse], q=(0.5,), skip_inf=True, out=rec[0:1])
        summarize(mv[i_rmse::i_kge - i_rmse][:2], q=(0.5,), out=rec[1:3])
        for k, (_, t) in enumerate(items):
            summarize(t, q=(0.5,), method="lower", out=rec[3 + k:4 + k])
    return StepSummary(rec, tuple(n for n, _ in items), tuple(int(t.numel()) for _, t in items))
