"""Stores, batches and expectations shared by test_feed_api.py (host halves) and test_gpu_feed.py (kernels).  Every
expected value is a NumPy restatement of the reference's host path, written here and never taken from the code under
test: ``StreamflowReader.forward`` (src/ddr/io/readers.py:461-531), the gauge-id padding of readers.py:558 and the
observation filter of scripts/train.py:84-92 over the window of io/builders.py:128.  Comparison is bitwise."""

from __future__ import annotations

from types import SimpleNamespace

import numpy as np

FILL = np.float32(0.001)  # torch.full(..., fill_value=0.001, dtype=torch.float32), readers.py:524-529
NO_VALID = "No valid divide IDs found in this batch. Throwing error"
SPECIAL = {"nan_days": 6, "all_nan": 7, "plus_inf": 8}  # store rows
NAN_DAYS = (0, 1, 5, 63, 64, 65, 129, 500, 1030)
INF_DAYS = (2, 64, 130, 1029)


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b) -> bool:
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(bits(a), bits(b))


def lognormal_store(n: int = 300, T: int = 1031, seed: int = 0) -> np.ndarray:
    """Seeded log-normal q' (random mantissas), with three special rows -- NaN at single days, NaN throughout, +inf
    at single days -- and, in row 9, a -0.0, a NaN with a payload and a signalling NaN, which a bitwise copy keeps."""
    rng = np.random.default_rng(seed)
    scale = rng.lognormal(np.log(0.5), 1.0, (n, 1))
    qr = (scale * rng.lognormal(0.0, 0.5, (n, T))).astype(np.float32)
    if n > 9:
        qr[SPECIAL["nan_days"], [d for d in NAN_DAYS if d < T]] = np.nan
        qr[SPECIAL["all_nan"]] = np.nan
        qr[SPECIAL["plus_inf"], [d for d in INF_DAYS if d < T]] = np.inf
        w = qr[9].view(np.uint32)
        w[0], w[min(3, T - 1)], w[T // 2] = 0x80000000, 0xFFC12345, 0x7FA00001
    return qr


def batch_rows(n_rows: int, N: int, seed: int) -> np.ndarray:
    """N store rows in random order (repeats when N > n_rows), the special rows and row 9 among them when N allows."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, n_rows, N).astype(np.int32)
    take = [*SPECIAL.values(), 9][: max(0, N - 1)]
    where = rng.choice(N, size=len(take), replace=False) if take else []
    rows[where] = take
    return rows


def expected_gather(qr, rows, t0: int, n_cols: int, repeat: int = 1, T_out: int | None = None):
    """``(out (T_out, N), valid (N,))``: readers.py:508-530 for rows that are already looked up; a row outside the
    store is a missing divide."""
    rows = np.asarray(rows, np.int64)
    T_out = n_cols * repeat if T_out is None else T_out
    ok = (rows >= 0) & (rows < qr.shape[0])
    sel = qr[rows[ok]][:, t0:t0 + n_cols]
    data = np.repeat(sel, repeat, axis=1)[:, :T_out].T
    out = np.full((T_out, len(rows)), FILL, np.float32)
    out[:, ok] = data
    return out, ok


def streamflow_reader(qr, store_ids, batch_ids, time_idx, is_hourly: bool, n_hourly: int) -> np.ndarray:
    """readers.py:477-531, line by line, on the NumPy store (``isel`` is the two fancy indices)."""
    lookup = {d: i for i, d in enumerate(store_ids)}
    valid_rows, mask = [], []
    for i, d in enumerate(batch_ids):
        if d in lookup:
            valid_rows.append(lookup[d])
            mask.append(i)
    assert len(valid_rows) != 0, NO_VALID
    time_idx = np.asarray(time_idx)
    assert time_idx[0] >= 0 and time_idx[-1] < qr.shape[1]
    ds = qr[np.asarray(valid_rows)][:, time_idx]
    if not is_hourly:
        data = np.repeat(ds.astype(np.float32), 24, axis=1)[:, :n_hourly].T
    else:
        data = ds.astype(np.float32).T
    out = np.full((data.shape[0], len(batch_ids)), FILL, np.float32)
    out[:, mask] = data
    return out


def expected_observations(store, rows, day0: int, n_days: int):
    """scripts/train.py:84-92: ``(target (G, n_days - 2), has_nan (G,))``; an unknown gauge is an all-NaN row."""
    rows = np.asarray(rows, np.int64)
    known = (rows >= 0) & (rows < store.shape[0])
    window = np.full((len(rows), n_days), np.nan, np.float32)
    window[known] = store[rows[known]][:, day0:day0 + n_days]
    return window[:, 1:-1].copy(), np.isnan(window).any(axis=1)


def dict_rows(store_ids, batch_ids) -> np.ndarray:
    """The reference's lookup (readers.py:455 and 480-485) with -1 for a miss."""
    lookup = {d: i for i, d in enumerate(store_ids)}
    return np.array([lookup.get(d, -1) for d in batch_ids], np.int32).reshape(-1)


def dates_like(first_day: int, rho: int) -> SimpleNamespace:
    """What the feed reads of the reference's ``Dates``: ``rho`` days from day ``first_day`` (counted from
    1980/01/01), and the hours of all of them but the last."""
    day0 = np.datetime64("1980-01-01", "D") + first_day
    hours = day0.astype("datetime64[h]") + np.arange((rho - 1) * 24)
    return SimpleNamespace(numerical_time_range=np.arange(first_day, first_day + rho),
                           batch_daily_time_range=day0 + np.arange(rho),
                           batch_hourly_time_range=hours.astype("datetime64[ns]"))


def ids_of(kind: str, numbers) -> list:
    return [f"cat-{i}" for i in numbers] if kind == "cat" else [int(i) for i in numbers]
