"""The summed-Q' baseline on the device (``csrc/summedq.hip``): per gauge and day, the sum of the lateral inflow of
the gauge's upstream divides, the unrouted series every routed result is scored against.

The reference computes it in ``scripts/summed_q_prime.py`` (``eval_q_prime``, lines 208-261): hourly stores are
collapsed to daily means on the host, then a Python loop does one ``np.isin`` over the store's divide ids and one
``cp.nansum(qr[idx], axis=0)`` per gauge, and the result goes to ``Metrics(pred, target)``.  Here

* :func:`members_from_ids` -- the host half (lines 192-205 and 258): the store's divide ids and each gauge's id
  list -> CSR member lists, one lookup for all gauges;
* :class:`SummedQPrime` -- the plan of those lists; calling it with the device-resident store gives the (G, D)
  daily series in one launch (two when a list is split), no host sync (capturable);
* :func:`summed_q_prime_metrics` -- that series handed straight to :func:`metrics_device`.

All sums run in fp64 over the fp32 store in list order and are rounded once: a gauge's row is bit-identical
whichever other gauges share the call, and within one fp32 rounding of the exact sum.
"""

from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _lib
from .metrics import metrics_device


def members_from_ids(row_ids, gauge_member_ids) -> tuple[np.ndarray, np.ndarray]:
    """``(off int64[G + 1], idx int32[nnz])``: for each gauge the rows of the store whose id is in the gauge's id
    list, ascending -- per gauge ``np.where(np.isin(row_ids, ids))[0]``, computed with one sort of ``row_ids`` for
    all gauges.  ``row_ids`` are integers or strings (``cat-123``); ids absent from the store are dropped."""
    row_ids = np.asarray(row_ids)
    if row_ids.ndim != 1:
        raise ValueError("row_ids must be 1-D")
    if row_ids.size > np.iinfo(np.int32).max:
        raise ValueError("too many rows for int32 indices")
    text = row_ids.dtype.kind in "USO"
    lists = []
    for ids in gauge_member_ids:
        a = np.asarray(ids).reshape(-1)
        lists.append(a.astype(str) if text else a)
    G = len(lists)
    counts = np.array([a.size for a in lists], np.int64)
    filled = [a for a in lists if a.size]
    if not filled or row_ids.size == 0:
        return np.zeros(G + 1, np.int64), np.zeros(0, np.int32)
    ids = np.concatenate(filled)
    gauge = np.repeat(np.arange(G, dtype=np.int64), counts)
    keys = row_ids.astype(str) if text else row_ids
    sorter = np.argsort(keys, kind="stable")
    ordered = keys[sorter]
    left = np.searchsorted(ordered, ids, "left")
    hits = np.searchsorted(ordered, ids, "right") - left  # rows carrying this id (0: absent from the store)
    total = int(hits.sum())
    start = np.cumsum(hits) - hits
    rows = sorter[np.repeat(left, hits) + (np.arange(total, dtype=np.int64) - np.repeat(start, hits))]
    gauge = np.repeat(gauge, hits)
    order = np.lexsort((rows, gauge))
    rows, gauge = rows[order], gauge[order]
    keep = np.ones(total, bool)  # (an id listed twice for a gauge selects its row once, as isin does)
    keep[1:] = (rows[1:] != rows[:-1]) | (gauge[1:] != gauge[:-1])
    rows, gauge = rows[keep], gauge[keep]
    off = np.zeros(G + 1, np.int64)
    np.cumsum(np.bincount(gauge, minlength=G), out=off[1:])
    return off, rows.astype(np.int32)


class SummedQPrime:
    """The plan of G member lists (``off`` int64[G + 1], ``idx`` int32[nnz]: gauge g sums rows
    ``idx[off[g]:off[g + 1]]`` in that order) on ``device`` (default: the current HIP device).

    ``summed(qr, hours_per_step=24)`` takes the lateral-inflow store as the reference holds it, a float32
    ``(n_rows, T)`` device tensor with time on the inner axis, and returns ``pred``, float32 ``(G, T //
    hours_per_step)``, on the current stream without a host sync.  Lists longer than ``chunk`` members are split
    across workgroups at multiples of ``chunk``."""

    def __init__(self, off, idx, device=None, chunk: int = 4096) -> None:
        off = np.ascontiguousarray(np.asarray(off), dtype=np.int64).reshape(-1)
        idx = np.ascontiguousarray(np.asarray(idx), dtype=np.int32).reshape(-1)
        if off.size < 1:
            raise ValueError("off must hold G + 1 offsets")
        if int(off[-1]) != idx.size:
            raise ValueError(f"off[-1] = {int(off[-1])} does not match the {idx.size} indices")
        self.n_gauges = off.size - 1
        self.chunk = int(chunk)
        self.max_index = int(idx.max()) if idx.size else -1
        self.device = None
        self._plan = C.c_void_p()
        lib = _lib.load()
        if torch.cuda.is_available():
            self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
            with torch.cuda.device(self.device):
                code = lib.ddr_summedq_plan_create(self.n_gauges, off.ctypes.data, idx.ctypes.data, self.chunk,
                                                   _lib.stream_ptr(self.device), C.byref(self._plan))
        else:  # (the plan still checks its lists; calling it raises)
            code = lib.ddr_summedq_plan_create(self.n_gauges, off.ctypes.data, idx.ctypes.data, self.chunk, None,
                                               C.byref(self._plan))
        _lib.check(code)

    def __del__(self) -> None:
        plan, self._plan = getattr(self, "_plan", None), None
        if plan:
            try:
                _lib.load().ddr_summedq_plan_destroy(plan)
            except Exception:  # noqa: BLE001  (interpreter shutdown)
                pass

    def scratch_bytes(self, n_days: int) -> int:
        """Bytes of fp64 partial rows a call with ``n_days`` days needs (0 when no list is split)."""
        return int(_lib.load().ddr_summedq_scratch_bytes(self._plan, n_days))

    def __call__(self, qr: torch.Tensor, hours_per_step: int = 24) -> torch.Tensor:
        if not isinstance(qr, torch.Tensor):
            raise TypeError("SummedQPrime takes a torch tensor")
        if qr.dtype != torch.float32:
            raise ValueError("qr must be float32")
        if qr.dim() != 2:
            raise ValueError("qr must be 2-D (n_rows, T)")
        if hours_per_step not in (1, 24):
            raise ValueError("hours_per_step must be 24 (hourly store) or 1 (daily store)")
        n_rows, T = qr.shape
        if T < hours_per_step:
            raise ValueError("qr holds less than one day")
        if n_rows <= self.max_index:
            raise ValueError(f"qr has {n_rows} rows, the member lists index row {self.max_index}")
        if not qr.is_cuda:
            raise RuntimeError("SummedQPrime runs on the HIP device only (no CPU fallback)")
        if qr.device != self.device:
            raise ValueError(f"qr is on {qr.device}, the plan on {self.device}")
        if qr.stride(1) != 1:
            qr = qr.contiguous()
        D = T // hours_per_step
        lib = _lib.load()
        with torch.cuda.device(self.device):
            pred = torch.empty((self.n_gauges, D), device=self.device, dtype=torch.float32)
            nbytes = self.scratch_bytes(D)
            scratch = torch.empty(nbytes // 8, device=self.device, dtype=torch.float64) if nbytes else None
            _lib.check(lib.ddr_summedq_f32(self._plan, qr.data_ptr(), n_rows, qr.stride(0), T, hours_per_step,
                                           pred.data_ptr(), D, _lib.ptr(scratch), nbytes,
                                           _lib.stream_ptr(self.device)))
        return pred


def summed_q_prime_metrics(summed: SummedQPrime, qr: torch.Tensor, target: torch.Tensor, hours_per_step: int = 24,
                           warmup: int = 0) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(pred, values, pred_nan_count)``: the summed-Q' series of ``qr`` and its 18 metrics against ``target``
    (:func:`metrics_device`), all on the device and the current stream; nothing is copied to the host between the
    q' store and the metrics."""
    pred = summed(qr, hours_per_step)
    values, count = metrics_device(pred, target, warmup)
    return pred, values, count
