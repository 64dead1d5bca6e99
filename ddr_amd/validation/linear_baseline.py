"""The fixed-parameter linear routing arm of the reference's ``benchmarks/`` package on the device.

The reference (``benchmarks/src/ddr_benchmarks/benchmark.py:121-234`` and ``:794-797``) routes every gauge's own
subgraph through DiffRoute's ``LTIRouter`` in a Python loop, with k = 0.1042 d, x = 0.3, dt = 1 h and a zero initial
state, takes the discharge of the gauge's reach, and pools the hourly series ``[13 + tau : -11 + tau]`` to days like
the DDR arm.  Here the union of the gauges' subnetworks is routed once (:class:`ddr_amd.routing.LinearMuskingum`):
a reach's discharge depends only on what lies upstream of it, so a gauge's row is bit-identical to its own
subnetwork routed alone.  Three deviations, all stated in INTEGRATION.md: RAPID's matrix scheme instead of
DiffRoute's truncated impulse-response convolution, one union route instead of per-gauge graphs, and headwater
gauges optionally routed instead of left as NaN.
"""

from __future__ import annotations

import numpy as np
import torch

from ..ops import GaugeMap
from ..routing.linear import MODELS, LinearMuskingum


def pooled_days(T: int, tau: int) -> tuple[int, int, int]:
    """``(a, b, D)``: the hourly slice ``[a:b]`` = ``[13 + tau : -11 + tau]`` of a T-hour series and the days
    ``len(series[13 : -11 + tau]) // 24`` it is pooled to (benchmark.py:787-797)."""
    end = T + (-11 + tau) if (-11 + tau) < 0 else min(T, -11 + tau)
    a, b = 13 + tau, end
    D = max(end - 13, 0) // 24
    if D < 1 or b - a < D:
        raise ValueError(f"T = {T} hours leaves no whole day after the [13 + tau : -11 + tau] trim")
    return a, b, D


def linear_baseline(index, gauges, store, rows, window, *, k_days: float = 0.1042, x: float = 0.3,
                    dt_days: float = 1.0 / 24.0, irf_fn: str = "muskingum", tau: int = 3,
                    skip_headwaters: bool = True, **graph_kw):
    """``(hourly (G, T), daily (G, D))`` float32 on the device: the linear baseline at ``gauges``.

    ``index``: a device :class:`ddr_amd.upstream.UpstreamIndex`; ``gauges``: the gauges' reach indices in it;
    ``store``: the :class:`ddr_amd.io.stores.StreamflowStore`; ``rows``: its rows of the whole domain
    (``store.align(conus_divide_ids)``); ``window``: ``(t0, T)``, the first store hour (or day, for a daily store:
    see ``StreamflowStore.hourly``) and the hours routed.  ``skip_headwaters`` leaves a gauge whose subnetwork has no
    edge as a NaN row, as the reference does (benchmark.py:186-189); ``False`` routes it.  ``graph_kw`` goes to the
    routing graph's builder.  The result goes to ``metrics_device`` / ``Metrics`` as it is."""
    if irf_fn not in MODELS:
        raise ValueError(f"irf_fn must be one of {MODELS} (the other DiffRoute IRFs are not implemented), not {irf_fn!r}")
    if index.device is None:
        raise RuntimeError("linear_baseline needs a device UpstreamIndex (no CPU fallback)")
    t0, T = int(window[0]), int(window[1])
    a, b, D = pooled_days(T, int(tau))
    gauges = np.asarray(gauges, np.int64).reshape(-1)
    db = index.collate(gauges)
    graph = db.graph(**graph_kw)
    q, _ = store.hourly(rows[db.active.long()], t0, T)  # (T, N): a divide the store lacks is filled with 0.001
    k = float(k_days) * 86400.0
    lm = LinearMuskingum(graph, k, None if irf_fn == "linear_storage" else float(x), dt=float(dt_days) * 86400.0,
                         substeps=1, model=irf_fn)
    gz = GaugeMap.build([np.array([int(c)]) for c in db.gage_c.cpu().numpy()], db.n, q.device)
    with torch.no_grad():
        hourly, _ = lm(q, output="end", gauges=gz)
    if skip_headwaters:
        down = index.down
        indeg = np.bincount(down[down >= 0], minlength=index.n)
        head = torch.from_numpy(indeg[gauges] == 0).to(hourly.device)
        hourly = torch.where(head[:, None], torch.full_like(hourly, float("nan")), hourly)
    daily = torch.nn.functional.interpolate(hourly[:, a:b].unsqueeze(1), size=(D,), mode="area").squeeze(1)
    return hourly, daily
