"""Whole-period inference on the device: chunked routing to daily discharge (``csrc/period.hip``).

What the reference's ``ddr route`` / ``ddr test`` do (``scripts/router.py:88-201``, ``scripts/test.py:57-112``): walk
the period in ``batch_size``-day chunks, every chunk after the first with the previous day prepended and
``carry_state=True``, copy each chunk's hourly output into a host array, trim it to ``[13 + tau : -11 + tau]`` and
pool it to daily means (``scripts_utils.compute_daily_runoff``).  The chunking is part of the result: chunk ``i > 0``
repeats the previous chunk's last hour as its column 0 and its step ``t`` consumes ``q'[t - 1]`` of the chunk, so a
port has to reproduce the plan exactly (:func:`period_chunks`).

:class:`PeriodRouter` runs that loop with one forward and one daily accumulation per chunk on the current stream:
no hourly array, no host synchronisation, only the ``(R, n_days - 2)`` daily series leaves the kernels.  The host half
(:func:`period_chunks`) needs no device.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import torch

from . import _lib
from .ops import GaugeMap, RouteConsts, _consts, _gauges, _reaches

TAU_RANGE = (0, 10)  # the trim [13 + tau : -11 + tau] keeps n_days - 2 whole days for these


def _check_tau(tau: int) -> int:
    tau = int(tau)
    if not TAU_RANGE[0] <= tau <= TAU_RANGE[1]:
        raise ValueError(f"tau = {tau} is outside [{TAU_RANGE[0]}, {TAU_RANGE[1]}]: the trim [13 + tau : -11 + tau] "
                         "must end before the period does")
    return tau


def period_chunks(n_days: int, chunk_days: int) -> list[tuple[int, int]]:
    """``(first_day, last_day)`` (inclusive) of every routed chunk of an ``n_days`` period.

    The reference's plan (``DataLoader(SequentialSampler, batch_size)`` and ``base_geodataset.py:44-49``): chunk
    ``k`` holds the day indices ``[k B, min((k + 1) B, n_days))``, with ``k B - 1`` prepended for ``k > 0``.  A chunk
    routes ``(last - first) * 24`` hours starting at period hour ``first * 24``; one of zero hours is skipped."""
    n_days, B = int(n_days), int(chunk_days)
    if B < 2:
        raise ValueError(f"chunk_days = {B}: a chunk needs at least 2 days (its last day is never routed)")
    if n_days < 3:
        raise ValueError(f"n_days = {n_days}: the trimmed period needs at least 3 days")
    out = []
    for s in range(0, n_days, B):
        first, last = (s - 1 if s > 0 else 0), min(s + B, n_days) - 1
        if last > first:
            out.append((first, last))
    return out


@dataclass
class PeriodResult:
    """``daily`` (R, n_days - 2): the daily means of the period's days 1 .. n_days - 2 (R gauges, or every reach in
    reference order); ``q_last`` / ``top_width`` / ``side_slope`` (N) of the last chunk; ``hourly`` (G,
    (n_days - 1) * 24) with ``keep_hourly``, else None."""

    daily: torch.Tensor
    q_last: torch.Tensor
    top_width: torch.Tensor
    side_slope: torch.Tensor
    hourly: torch.Tensor | None = None

    def metrics(self, target, warmup: int = 0):
        """``validation.Metrics`` of ``daily[:, warmup:]`` against ``target[:, warmup:]``, on the device."""
        from .validation.metrics import Metrics

        w = int(warmup)
        if not isinstance(target, torch.Tensor):
            target = torch.as_tensor(target)
        target = target.to(self.daily.device)
        if target.shape != self.daily.shape:
            raise ValueError(f"target is {tuple(target.shape)}, the daily series {tuple(self.daily.shape)}")
        return Metrics(pred=self.daily[:, w:].float().contiguous(), target=target[:, w:].float().contiguous())

    def metrics_from(self, obs_store, rows: torch.Tensor, day0: int, warmup: int = 0):
        """:meth:`metrics` against the observations of days ``1 .. n_days - 2`` of the period (``test.py:77``,
        ``obs[:, 1:-1]``) taken from an ``ObservationStore`` whose column ``day0`` is the period's first day."""
        target, _ = obs_store.window(rows, int(day0), self.daily.shape[1] + 2)
        return self.metrics(target, warmup)


class PeriodRouter:
    """Route a whole period chunk by chunk and keep only its daily discharge.

    ``graph`` is the (unsplit) :class:`RiverGraph`; ``length`` / ``slope`` / ``x_storage`` the per-reach statics;
    ``gauges`` a :class:`GaugeMap` (or ``outflow_idx`` lists) for gauge rows, None for every reach; ``tau`` and
    ``chunk_days`` the reference's ``cfg.params.tau`` and ``batch_size``.  ``math`` as in :func:`ops.route`."""

    def __init__(self, graph, length, slope, x_storage, *, gauges=None, flow_scale=None,
                 consts: RouteConsts = RouteConsts(), tau: int = 3, chunk_days: int, math: str = "exact"):
        self.tau = _check_tau(tau)
        self.chunk_days = int(chunk_days)
        if self.chunk_days < 2:
            raise ValueError(f"chunk_days = {chunk_days}: a chunk needs at least 2 days")
        if math not in ("exact", "faithful", "fast"):
            raise ValueError(f"math must be 'exact', 'faithful' or 'fast', not {math!r}")
        self.graph = graph
        self.length, self.slope, self.x_storage, self.flow_scale = length, slope, x_storage, flow_scale
        if gauges is not None and not isinstance(gauges, GaugeMap):
            gauges = GaugeMap.build(gauges, graph.n, length.device)
        self.gauges = gauges
        self.consts = consts
        self.math = math

    # ------------------------------------------------------------------------------------------
    def _source(self, source, n_days: int, N: int):
        """-> (kind, payload, dtype, device): kind "daily" / "hourly" (tensor, valid) or "store" (store, rows, day0)."""
        if isinstance(source, tuple) and len(source) == 3:
            store, rows, day0 = source
            day0 = int(day0)
            rows = store._check_rows(rows)
            if rows.numel() != N:
                raise ValueError(f"rows has {rows.numel()} entries, the network has {N} reaches")
            per = store.hours_per_column
            need = n_days if per == 24 else (n_days - 1) * 24
            store._check_window(day0 * (24 // per), need)
            return "store", (store, rows, day0), torch.float32, store.device
        valid = None
        if isinstance(source, tuple) and len(source) == 2:
            source, valid = source
        if not isinstance(source, torch.Tensor):
            raise TypeError("source must be a tensor, (tensor, valid) or (StreamflowStore, rows, day0)")
        if not source.is_cuda:
            raise RuntimeError("period inference runs on the HIP device only (no CPU fallback); move the source to cuda")
        if source.dtype not in (torch.float32, torch.float64):
            raise TypeError("routing supports float32 and float64")
        if source.dim() != 2 or source.shape[1] != N:
            raise ValueError(f"source must be (rows, {N}), not {tuple(source.shape)}")
        if source.shape[0] == n_days:
            kind = "daily"
        elif source.shape[0] == (n_days - 1) * 24:
            kind = "hourly"
        else:
            raise ValueError(f"source has {source.shape[0]} rows: a period of {n_days} days needs {n_days} daily or "
                             f"{(n_days - 1) * 24} hourly rows")
        if valid is not None:
            if valid.numel() != N:
                raise ValueError("valid must be a mask of N reaches")
            valid = valid.to(device=source.device, dtype=torch.uint8).contiguous()
        return kind, (source.detach().contiguous(), valid), source.dtype, source.device

    def _window(self, kind, payload, first: int, last: int):
        """-> (q' tensor, valid, qprime_hours) of the chunk (first, last)."""
        T = (last - first) * 24
        if kind == "store":
            store, rows, day0 = payload
            if store.hours_per_column == 24:
                qd, valid = store.daily(rows, day0 + first, last - first + 1)
                return qd, valid.to(torch.uint8), 24
            qh, valid = store.hourly(rows, (day0 + first) * 24, T)
            return qh, valid.to(torch.uint8), 1
        src, valid = payload
        if kind == "daily":
            return src[first:last + 1], valid, 24
        return src[first * 24:last * 24], valid, 1

    @torch.no_grad()
    def run(self, n, q_spatial, p_spatial, source, n_days: int, *, keep_hourly: bool = False) -> PeriodResult:
        """Route ``n_days`` days from ``source`` -- a daily tensor ``(n_days, N)`` (or ``(tensor, valid)``), an hourly
        tensor ``((n_days - 1) * 24, N)``, or ``(StreamflowStore, rows, day0)`` -- and return the daily series.

        One forward (no runoff output, ``q0`` = the previous chunk's ``q_last``) and one daily accumulation per chunk,
        all on the current stream; workspaces are sized for the largest chunk and reused."""
        g = self.graph
        n_days = int(n_days)
        chunks = period_chunks(n_days, self.chunk_days)
        gz = self.gauges
        if keep_hourly and gz is None:
            raise ValueError("keep_hourly needs gauge mode: hourly all-segment output is not kept on the device")
        N = g.n
        kind, payload, dt, dev = self._source(source, n_days, N)
        f32 = dt == torch.float32

        def prep(t):
            return None if t is None else t.detach().to(device=dev, dtype=dt).contiguous()

        n, q, p, length, slope, x_storage, flow_scale = map(
            prep, (n, q_spatial, p_spatial, self.length, self.slope, self.x_storage, self.flow_scale))
        p = p.reshape(-1) if p.numel() > 1 else p.reshape(1)
        for name, t in (("n", n), ("q_spatial", q), ("length", length), ("slope", slope), ("x_storage", x_storage),
                        ("flow_scale", flow_scale)):
            if t is not None and t.numel() != N:
                raise ValueError(f"{name} has {t.numel()} elements, the network has {N} reaches")
        if p.numel() not in (1, N):
            raise ValueError(f"p_spatial has {p.numel()} elements: expected 1 or {N}")

        lib = _lib.load()
        fwd = lib.ddr_mc_forward_f32 if f32 else lib.ddr_mc_forward_f64
        acc = lib.ddr_period_daily_f32 if f32 else lib.ddr_period_daily_f64
        red = lib.ddr_gauge_reduce_f32 if f32 else lib.ddr_gauge_reduce_f64
        D, H, first_hour = n_days - 2, (n_days - 1) * 24, 13 + self.tau
        R = gz.n_gauges if gz is not None else N
        T_max = max((last - first) * 24 for first, last in chunks)
        with torch.cuda.device(dev):
            stream = _lib.stream_ptr(dev)
            x_save = torch.empty(g.save_numel(T_max), device=dev, dtype=dt)
            bnd = torch.empty(g.bnd_numel(T_max), device=dev, dtype=torch.float64)
            daily = torch.empty((R, D), device=dev, dtype=dt)
            state = [torch.empty(N, device=dev, dtype=dt) for _ in range(2)]
            tw = torch.zeros(N, device=dev, dtype=dt)
            ss = torch.zeros(N, device=dev, dtype=dt)
            hourly = torch.empty((R, H), device=dev, dtype=dt) if keep_hourly else None
            gzc = _gauges(R, gz.offsets, gz.index, None, None) if gz is not None else None
            gref = C.byref(gzc) if gzc is not None else None
            c = _consts(self.consts.as_list())
            qlb = float(self.consts.discharge_lb)
            base = (_lib.DDR_FWD_NO_RUNOFF | (_lib.DDR_FWD_FAST_MATH if self.math == "fast" else 0)
                    | (_lib.DDR_FWD_FAITHFUL_MATH if self.math == "faithful" else 0))
            # argument check without a launch (a split or host-only graph raises here): a range no day's window meets
            _lib.check(acc(g.handle, x_save.data_ptr(), 1, gref, qlb, 0, first_hour + 24 * D, first_hour, D,
                           daily.data_ptr(), stream))
            q_last = None
            for i, (first, last) in enumerate(chunks):
                T = (last - first) * 24
                qp, valid, hours = self._window(kind, payload, first, last)
                flags = base | (_lib.DDR_FWD_CARRY if q_last is not None else 0)
                out = state[i & 1]
                status = torch.empty(g.info.status_bytes, device=dev, dtype=torch.uint8)
                r = _reaches(n, q, p, length, slope, x_storage, flow_scale, hours, valid)
                _lib.check(fwd(g.handle, C.byref(c), C.byref(r), qp.data_ptr(), T, _lib.ptr(q_last), None,
                               x_save.data_ptr(), bnd.data_ptr() if bnd.numel() else None, status.data_ptr(),
                               out.data_ptr(), tw.data_ptr(), ss.data_ptr(), int(flags), stream))
                _lib.check(acc(g.handle, x_save.data_ptr(), T, gref, qlb, int(flags), first * 24, first_hour, D,
                               daily.data_ptr(), stream))
                if keep_hourly:
                    # the chunk's (G, T) hourly series, then into its columns of the period's
                    part = torch.empty((R, T), device=dev, dtype=dt)
                    _lib.check(red(g.handle, x_save.data_ptr(), T, gref, qlb, int(flags), part.data_ptr(), stream))
                    hourly[:, first * 24:last * 24] = part
                q_last = out
        return PeriodResult(daily, q_last, tw, ss, hourly)
