"""NaN-aware summaries of long rows on the device (``csrc/summary.hip``, ``ddr_summary_f32`` / ``ddr_summary_f64``).

The reference takes order statistics on the host: ``np.nanpercentile`` over every attribute of the store
(``io/statistics.py:45-52``), ``np.nanmedian`` over the gauges' metrics (``validation/utils.py:110-112``) and
``torch.median`` over each routing parameter after a ``.cpu()`` per step (``scripts/train.py:127-131``).
:func:`summarize` gives, per row, the count of the values that take part, their min, max, mean, population std and
up to eight quantiles, exactly (radix selection over order-preserving keys: nothing is sorted), in fp64, with no
host synchronisation, allocation or copy inside the call, so a captured step can hold it.
"""

from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import torch

from . import _lib

#: the columns of :attr:`Summary.table` before the quantiles (``DDR_SUMMARY_*`` in ``include/ddr_mc.h``)
SUMMARY_COLUMNS = _lib.SUMMARY_COLUMNS
#: ``method=`` of :func:`summarize` (``DDR_SUMMARY_LINEAR``, ``DDR_SUMMARY_LOWER``)
SUMMARY_METHODS = _lib.SUMMARY_METHODS
SUMMARY_SKIP_INF = _lib.SUMMARY_SKIP_INF
#: quantiles per call at most (``DDR_SUMMARY_MAX_Q``)
MAX_QUANTILES = _lib.SUMMARY_MAX_Q
#: elements of a row that one workgroup takes at a time (``DDR_SUMMARY_TILE``)
TILE = _lib.SUMMARY_TILE


@dataclass
class Summary:
    """One :func:`summarize` call: ``table`` is the (R, 5 + K) fp64 device tensor, the rest are views of it."""

    table: torch.Tensor

    @property
    def count(self) -> torch.Tensor:
        return self.table[:, 0]

    @property
    def min(self) -> torch.Tensor:
        return self.table[:, 1]

    @property
    def max(self) -> torch.Tensor:
        return self.table[:, 2]

    @property
    def mean(self) -> torch.Tensor:
        return self.table[:, 3]

    @property
    def std(self) -> torch.Tensor:
        return self.table[:, 4]

    @property
    def quantiles(self) -> torch.Tensor:
        """(R, K), in the order of ``q``."""
        return self.table[:, len(SUMMARY_COLUMNS):]


def _check_q(q) -> tuple[float, ...]:
    try:
        q = tuple(float(v) for v in (q if hasattr(q, "__iter__") else (q,)))
    except (TypeError, ValueError) as e:
        raise ValueError(f"q must be a sequence of probabilities: {e}") from None
    if len(q) > MAX_QUANTILES:
        raise ValueError(f"at most {MAX_QUANTILES} quantiles per call, not {len(q)}")
    for v in q:
        if math.isnan(v) or not 0.0 <= v <= 1.0:
            raise ValueError(f"q must lie in [0, 1], not {v}")
    return q


def summarize(x: torch.Tensor, q=(), *, method: str = "linear", skip_inf: bool = False,
              out: torch.Tensor | None = None) -> Summary:
    """Per row of a (N,) or (R, N) fp32 or fp64 HIP tensor: count, min, max, mean, std (ddof = 0, two-pass) and the
    quantiles at the probabilities ``q`` (at most 8), as fp64.

    NaN never takes part; with ``skip_inf`` neither does +-inf.  A row in which nothing takes part has count 0 and
    NaN elsewhere.  ``method="linear"`` is ``np.nanquantile``'s default, evaluated in fp64 on the row's own values
    (for a fp32 row: ``np.nanquantile(x.astype(np.float64), q)``); ``method="lower"`` is the order statistic
    floor((n - 1) q), which at q = 0.5 is ``torch.median``'s element.  The order statistics are exact.

    Rows of any stride are read in place; a tensor whose innermost stride is not 1 is made contiguous.  ``out`` is a
    contiguous (R, 5 + K) fp64 tensor on ``x``'s device to write into (a captured step keeps it).  The launches go on
    the current stream: no host sync, no copy.  (The scratch buffer is a tensor of PyTorch's caching allocator, as in
    :func:`ddr_amd.train.daily_objective`: under capture it comes from the graph's pool.)  HIP device only."""
    if not isinstance(x, torch.Tensor):
        raise TypeError("summarize takes a torch tensor")
    if x.dtype not in (torch.float32, torch.float64):
        raise ValueError("x must be float32 or float64")
    if x.dim() not in (1, 2):
        raise ValueError("x must be a (N,) or (R, N) tensor")
    if method not in SUMMARY_METHODS:
        raise ValueError(f"method must be one of {SUMMARY_METHODS}, not {method!r}")
    q = _check_q(q)
    if x.dim() == 1:
        x = x.unsqueeze(0)
    R, N = x.shape
    if N >= 2 ** 31:
        raise ValueError("rows must be shorter than 2^31 values")
    cols = len(SUMMARY_COLUMNS) + len(q)
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or out.shape != (R, cols) \
                or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous ({R}, {cols}) float64 tensor")
        if out.device != x.device:
            raise ValueError("out must be on x's device")
    if not x.is_cuda:
        raise RuntimeError("summarize runs on the HIP device only (no CPU fallback)")
    x = x.detach()
    if N > 1 and x.stride(1) != 1:
        x = x.contiguous()
    stride = x.stride(0) if R > 1 else N
    if stride < 0:
        x, stride = x.contiguous(), N
    lib = _lib.load()
    with torch.cuda.device(x.device):
        table = out if out is not None else torch.empty((R, cols), device=x.device, dtype=torch.float64)
        if R:
            work = torch.empty(int(lib.ddr_summary_work_bytes(R, len(q), x.element_size())), device=x.device,
                               dtype=torch.uint8)
            fn = lib.ddr_summary_f32 if x.dtype == torch.float32 else lib.ddr_summary_f64
            qa = (C.c_double * max(1, len(q)))(*q)
            _lib.check(fn(R, N, x.data_ptr(), stride, len(q), qa, SUMMARY_METHODS.index(method),
                          SUMMARY_SKIP_INF if skip_inf else 0, table.data_ptr(), work.data_ptr(),
                          _lib.stream_ptr(x.device)))
    return Summary(table)
