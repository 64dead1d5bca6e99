"""Device-resident forcing stores and their per-batch feed (``csrc/feed.hip``).

The reference reads a batch's lateral inflow in ``StreamflowReader.forward`` (``src/ddr/io/readers.py:461-531``): a
Python loop of dict lookups over the batch's divide ids, an xarray ``isel`` of (divides x days), ``np.repeat(..., 24)``,
a transpose and the upload of a (T, N) tensor; the batch's observations are selected by xarray
(``io/builders.py:112-129``), NaN-filtered per gauge and trimmed on the host (``scripts/train.py:84-92``).  Here

* :class:`StreamflowStore` -- ``ds["Qr"].values`` uploaded once; ``rows`` / ``align`` map ids to store rows (one
  vectorised host lookup and one upload, or none for a batch collated on the device: ``aligned[db.active]``);
  ``daily`` gathers the batch's window into the (days, N) layout ``ops.route(..., qprime_hours=24,
  qprime_valid=valid)`` reads; calling the store like the reference's reader gives the same (T, N) tensor;
* :class:`ObservationStore` -- the gauge observations uploaded once; ``window`` returns the trimmed targets and the
  per-gauge "has a NaN" flag.

Gathers run on the current stream and never synchronise with the host; values are copied as bits.  There is no CPU
fallback: a host store raises ``RuntimeError``.  The host halves (:class:`RowIndex`, :func:`daily_window`,
:func:`hourly_window`, :func:`feed_plan`) need no device.
"""

from __future__ import annotations

import warnings

import numpy as np
import torch

from .. import _lib

FILL = 0.001  # a divide the store lacks carries minimum flow (readers.py:523-530)
ORIGIN = np.datetime64("1980-01-01", "s")  # the origin of Dates.numerical_time_range
NO_VALID_DIVIDES = "No valid divide IDs found in this batch. Throwing error"  # (readers.py:487)


def _timestamp(t) -> np.datetime64:
    """``t`` (``"1980/01/01"``, an ISO string, ``datetime``, ``np.datetime64``, ``pd.Timestamp``) in seconds."""
    if hasattr(t, "to_datetime64"):
        t = t.to_datetime64()
    if isinstance(t, str):
        date, _, clock = t.strip().replace("/", "-").replace("T", " ").partition(" ")
        y, m, d = (int(x) for x in date.split("-"))
        t = f"{y:04d}-{m:02d}-{d:02d}" + (f"T{clock}" if clock else "")
    return np.datetime64(t, "s")


class RowIndex:
    """The reference's ``{id: row for row, id in enumerate(ids)}`` (readers.py:455) as one sort: ``lookup(ids)``
    gives the int32 row of every id and -1 for an id the store lacks.  Ids are integers (MERIT COMIDs) or strings
    (``cat-123``); as in the dict, the last row carrying a repeated id wins."""

    def __init__(self, ids) -> None:
        ids = np.asarray(ids)
        if ids.ndim != 1:
            raise ValueError("ids must be 1-D")
        if ids.size > np.iinfo(np.int32).max:
            raise ValueError("too many rows for int32 indices")
        self.text = ids.dtype.kind in "USO"
        if not self.text and ids.dtype.kind not in "iu" and ids.size:
            raise TypeError(f"ids must be integers or strings, not {ids.dtype}")
        keys = ids.astype(str) if self.text else ids.astype(np.int64)
        self._sorter = np.argsort(keys, kind="stable")
        self._ordered = keys[self._sorter]

    def __len__(self) -> int:
        return self._ordered.size

    def lookup(self, ids) -> np.ndarray:
        ids = np.asarray(ids).reshape(-1)
        if ids.size == 0 or self._ordered.size == 0:
            return np.full(ids.size, -1, np.int32)
        if self.text:
            ids = ids.astype(str)
        elif ids.dtype.kind not in "iu":
            raise TypeError(f"the store's ids are integers, the batch's are {ids.dtype}")
        pos = np.searchsorted(self._ordered, ids, "right") - 1
        hit = (pos >= 0) & (self._ordered[np.maximum(pos, 0)] == ids)
        return np.where(hit, self._sorter[np.maximum(pos, 0)], -1).astype(np.int32)


def pad_gage_ids(ids) -> np.ndarray:
    """Gauge ids as the reference keys them: ``str(id).zfill(8)`` (readers.py:558)."""
    return np.array([str(g).zfill(8) for g in np.asarray(ids).reshape(-1).tolist()], dtype=str)


def _contiguous(first: int, last: int, count: int, what: str) -> None:
    if last - first != count - 1:
        raise ValueError(f"{what} is not a contiguous range ({count} entries from {first} to {last})")


def daily_window(dates, start) -> tuple[int, int, int]:
    """``(d0, n_days, T)`` of a batch against a daily store whose first day is ``start``: the store column of
    ``dates.numerical_time_range[0]`` (days since 1980/01/01, readers.py:459 and 497), the days the batch spans and
    ``T = len(dates.batch_hourly_time_range)`` (``(n_days - 1) * 24`` for the reference's ``Dates``)."""
    days = np.asarray(dates.numerical_time_range).reshape(-1)
    if days.size == 0:
        raise ValueError("dates.numerical_time_range is empty")
    first, last = int(days[0]), int(days[-1])
    _contiguous(first, last, days.size, "dates.numerical_time_range")
    offset = int((_timestamp(start) - ORIGIN) // np.timedelta64(86400, "s"))
    return first - offset, int(days.size), len(dates.batch_hourly_time_range)


def hourly_window(dates, start) -> tuple[int, int]:
    """``(h0, T)`` of a batch against an hourly store whose first hour is ``start``: whole hours from ``start`` to
    ``dates.batch_hourly_time_range[0]`` (readers.py:491-494) and the number of hours."""
    hours = np.asarray(dates.batch_hourly_time_range, dtype="datetime64[s]").reshape(-1)
    if hours.size == 0:
        raise ValueError("dates.batch_hourly_time_range is empty")
    t0 = _timestamp(start)
    first, last = (int((h - t0) // np.timedelta64(3600, "s")) for h in (hours[0], hours[-1]))
    _contiguous(first, last, hours.size, "dates.batch_hourly_time_range")
    return first, int(hours.size)


def feed_plan(index: RowIndex, start, is_hourly: bool, n_store_cols: int, routing_dataclass):
    """The host half of the drop-in call: ``(rows int32 (N,), t0, n_cols, repeat, T)`` for
    ``routing_dataclass.divide_ids`` and ``.dates``.  Raises the reference's ``AssertionError`` when the store holds
    none of the batch's divides, and ``ValueError`` when the batch's window leaves the store (the reference asserts,
    readers.py:499-506)."""
    rows = index.lookup(routing_dataclass.divide_ids)
    assert bool((rows >= 0).any()), NO_VALID_DIVIDES
    dates = routing_dataclass.dates
    if is_hourly:
        t0, T = hourly_window(dates, start)
        n_cols, repeat, span, unit = T, 1, T, "hours"
    else:
        t0, span, T = daily_window(dates, start)
        n_cols, repeat, unit = -(-T // 24), 24, "days"
        if n_cols > span:
            raise ValueError(f"{T} hourly steps need {n_cols} days, dates.numerical_time_range holds {span}")
    if t0 < 0 or t0 + span > n_store_cols:
        raise ValueError(f"the batch asks for {unit} [{t0}, {t0 + span}) counted from the store's start "
                         f"({_timestamp(start)}), the store holds [0, {n_store_cols})")
    return rows, t0, n_cols, repeat, T


def _device_of(device) -> torch.device:
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"the forcing stores live on the HIP device only (no CPU fallback), not on {device}")
    if not torch.cuda.is_available():
        raise RuntimeError("the forcing stores need a HIP device (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device()) if device.index is None else device


def _upload(values, n_ids: int, device, name: str) -> torch.Tensor:
    """The (n_rows, T) float32 store on the device: a NumPy array is uploaded once, a device tensor is kept."""
    if not isinstance(values, (np.ndarray, torch.Tensor)):
        raise TypeError(f"{name} must be a NumPy array or a torch tensor")
    if values.dtype not in (np.float32, torch.float32):
        raise ValueError(f"{name} must be float32, not {values.dtype}")
    if values.ndim != 2:
        raise ValueError(f"{name} must be 2-D (rows, time)")
    if values.shape[0] != n_ids:
        raise ValueError(f"{name} has {values.shape[0]} rows for {n_ids} ids")
    if isinstance(values, np.ndarray):
        device = _device_of(device)
        with warnings.catch_warnings():  # (a read-only array, e.g. a memory map: it is only read)
            warnings.simplefilter("ignore", UserWarning)
            return torch.from_numpy(np.ascontiguousarray(values)).to(device)
    if not values.is_cuda:
        raise RuntimeError(f"{name} is a host tensor: the forcing stores live on the HIP device only (no CPU "
                           "fallback)")
    if values.shape[1] > 1 and values.stride(1) != 1:
        raise ValueError(f"{name} must hold time on the inner axis (stride(1) == 1)")
    if values.shape[0] > 1 and values.stride(0) < values.shape[1]:
        raise ValueError(f"{name}'s rows overlap (stride(0) < T)")
    return values.detach()


class _Store:
    """A (n_rows, T) float32 device store with the ids of its rows."""

    def __init__(self, values, ids, start, device, name: str) -> None:
        self.index = RowIndex(ids)
        self.start = _timestamp(start)
        self.data = _upload(values, len(self.index), device, name)
        self.device = self.data.device
        self.n_rows, self.n_cols = self.data.shape
        self._stride = max(self.data.stride(0), self.n_cols) if self.n_rows > 1 else self.n_cols

    @property
    def day_offset(self) -> int:
        """Days from 1980/01/01 to the store's start (readers.py:459)."""
        return int((self.start - ORIGIN) // np.timedelta64(86400, "s"))

    def _to_device(self, rows: np.ndarray) -> torch.Tensor:
        return torch.from_numpy(rows).to(self.device)

    def _check_rows(self, rows) -> torch.Tensor:
        if not isinstance(rows, torch.Tensor):
            raise TypeError("rows must be a torch tensor (see rows() / align())")
        if rows.dtype != torch.int32:
            raise ValueError(f"rows must be int32, not {rows.dtype}")
        if rows.dim() != 1:
            raise ValueError("rows must be 1-D")
        if not rows.is_cuda:
            raise RuntimeError("rows is a host tensor: the feed runs on the HIP device only (no CPU fallback)")
        if rows.device != self.device:
            raise ValueError(f"rows is on {rows.device}, the store on {self.device}")
        return rows.contiguous()

    def _check_window(self, t0: int, n: int, least: int = 0) -> tuple[int, int]:
        t0, n = int(t0), int(n)
        if n < least:
            raise ValueError(f"a window of {n} columns is shorter than {least}")
        if t0 < 0 or t0 + n > self.n_cols:
            raise ValueError(f"the window [{t0}, {t0 + n}) leaves the store's [0, {self.n_cols})")
        return t0, n

    def __repr__(self) -> str:
        return f"{type(self).__name__}({self.n_rows} rows x {self.n_cols}, start {self.start}, {self.device})"


class StreamflowStore(_Store):
    """The lateral-inflow (q') store on the device.

    ``qr`` is ``ds["Qr"].values`` as the reference holds it -- float32 ``(n_divides, T_store)``, time on the inner
    axis -- as a NumPy array (uploaded once) or a device tensor (any row stride, ``stride(1) == 1``); ``divide_ids``
    its rows' ids; ``start`` its first timestamp; ``is_hourly`` as ``cfg.data_sources.is_hourly``."""

    def __init__(self, qr, divide_ids, start="1980/01/01", is_hourly: bool = False, device="cuda") -> None:
        super().__init__(qr, divide_ids, start, device, "qr")
        self.is_hourly = bool(is_hourly)

    @property
    def qr(self) -> torch.Tensor:
        return self.data

    @property
    def hours_per_column(self) -> int:
        """``qprime_hours`` of ``ops.route`` for what :meth:`daily` returns."""
        return 1 if self.is_hourly else 24

    def rows(self, divide_ids) -> torch.Tensor:
        """int32 ``(N,)`` on the device: the store row of every divide, -1 where the store lacks it
        (readers.py:480-485)."""
        return self._to_device(self.index.lookup(divide_ids))

    def align(self, conus_divide_ids) -> torch.Tensor:
        """:meth:`rows` of the whole domain, built once: a batch collated on the device (``UpstreamIndex.collate``)
        gets its rows as ``aligned[db.active]`` with no host step."""
        return self.rows(conus_divide_ids)

    def window_of(self, dates) -> tuple[int, int, int]:
        """``(t0, n_cols, T)`` for :meth:`daily` from a ``Dates``-like object: the store column the batch starts at,
        the columns it reads (days without the last one, or hours) and the hourly steps it routes."""
        if self.is_hourly:
            t0, T = hourly_window(dates, self.start)
            return t0, T, T
        d0, _, T = daily_window(dates, self.start)
        return d0, -(-T // 24), T

    def _gather(self, rows: torch.Tensor, t0: int, n_cols: int, repeat: int, T_out: int):
        N = rows.numel()
        with torch.cuda.device(self.device):
            out = torch.empty((T_out, N), device=self.device, dtype=torch.float32)
            valid = torch.empty((N,), device=self.device, dtype=torch.bool)
            _lib.check(_lib.load().ddr_feed_qprime_f32(
                self.data.data_ptr(), self._stride, self.n_rows, self.n_cols, rows.data_ptr(), N, t0, n_cols, repeat,
                T_out, FILL, out.data_ptr(), valid.data_ptr(), _lib.stream_ptr(self.device)))
        return out, valid

    def daily(self, rows: torch.Tensor, day0: int, n_days: int) -> tuple[torch.Tensor, torch.Tensor]:
        """``(qd, valid)``: ``qd`` float32 ``(n_days, N)`` with ``qd[d, i] = qr[rows[i], day0 + d]`` and 0.001 where
        ``rows[i]`` is not a row of the store (readers.py:523-530); ``valid`` bool ``(N,)``.  The input of
        ``ops.route(graph, qd, ..., qprime_hours=24, steps=T, qprime_valid=valid)``; for an hourly store pass the
        hour offset and count, and ``qprime_hours=1``."""
        rows = self._check_rows(rows)
        day0, n_days = self._check_window(day0, n_days)
        return self._gather(rows, day0, n_days, 1, n_days)

    def hourly(self, rows: torch.Tensor, t0: int, T: int) -> tuple[torch.Tensor, torch.Tensor]:
        """``(q, valid)``: the hourly (T, N) lateral inflow of looked-up ``rows`` from store column ``t0`` on -- the
        drop-in call without its host lookups.  A daily store is expanded in the kernel, ``q[t, i] = qr[rows[i],
        t0 + t // 24]``; an hourly store is copied."""
        rows = self._check_rows(rows)
        T = int(T)
        repeat = self.hours_per_column
        t0, n_cols = self._check_window(t0, -(-T // repeat))
        return self._gather(rows, t0, n_cols, repeat, T)

    def __call__(self, **kwargs) -> torch.Tensor:
        """The reference's ``flow(routing_dataclass=..., device=..., dtype=torch.float32)``: the (T, N) hourly
        lateral inflow of the batch, ``T = len(dates.batch_hourly_time_range)``.  A daily store is expanded in the
        kernel (``out[t, i] = qr[row_i, d0 + t // 24]``; the window's last day is never read)."""
        routing_dataclass = kwargs["routing_dataclass"]
        device = kwargs.get("device")
        if kwargs.get("dtype", torch.float32) != torch.float32:
            raise ValueError("the feed returns float32")
        if device is not None and _device_of(device) != self.device:
            raise ValueError(f"the store is on {self.device}, not on {device}")
        rows, t0, n_cols, repeat, T = feed_plan(self.index, self.start, self.is_hourly, self.n_cols, routing_dataclass)
        return self._gather(self._to_device(rows), t0, n_cols, repeat, T)[0]

    forward = __call__


class ObservationStore(_Store):
    """The gauge observations on the device: ``streamflow`` float32 ``(n_gauges, T_days)`` with NaN for a missing
    day, ``gage_ids`` its rows (keyed zero-filled to 8 digits, readers.py:558), ``start`` its first day."""

    def __init__(self, streamflow, gage_ids, start="1980/01/01", device="cuda") -> None:
        super().__init__(streamflow, pad_gage_ids(gage_ids), start, device, "streamflow")

    def rows(self, gage_ids) -> torch.Tensor:
        """int32 ``(G,)`` on the device: the store row of every gauge, -1 for an unknown one."""
        return self._to_device(self.index.lookup(pad_gage_ids(gage_ids)))

    def window_of(self, dates) -> tuple[int, int]:
        """``(day0, n_days)`` for :meth:`window`: the days of ``dates.batch_daily_time_range`` (builders.py:128)."""
        d0, n_days, _ = daily_window(dates, self.start)
        return d0, n_days

    def window(self, rows: torch.Tensor, day0: int, n_days: int) -> tuple[torch.Tensor, torch.Tensor]:
        """``(target, has_nan)`` of the window ``[day0, day0 + n_days)`` (scripts/train.py:84-92): ``target`` float32
        ``(G, n_days - 2)``, the window without its first and last day; ``has_nan`` bool ``(G,)``, true when any of
        the ``n_days`` days is NaN.  An unknown gauge is an all-NaN row.  The caller keeps ``~has_nan``."""
        rows = self._check_rows(rows)
        day0, n_days = self._check_window(day0, n_days, least=2)
        G = rows.numel()
        with torch.cuda.device(self.device):
            target = torch.empty((G, n_days - 2), device=self.device, dtype=torch.float32)
            has_nan = torch.empty((G,), device=self.device, dtype=torch.bool)
            _lib.check(_lib.load().ddr_feed_rows_f32(
                self.data.data_ptr(), self._stride, self.n_rows, self.n_cols, rows.data_ptr(), G, day0, n_days, 1,
                target.data_ptr(), n_days - 2, has_nan.data_ptr(), _lib.stream_ptr(self.device)))
        return target, has_nan
