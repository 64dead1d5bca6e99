"""The forcing feed without a GPU: the id lookups against the reference's dict, the window arithmetic, the Python
argument checks and the C ABI's declarations and refusals."""

import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import feed_cases as F
from ddr_amd import _lib
from ddr_amd.io import (ObservationStore, RowIndex, StreamflowStore, daily_window, feed_plan, hourly_window,
                        pad_gage_ids)

HEADER = Path(__file__).resolve().parents[1] / "include" / "ddr_mc.h"
FUNCTIONS = ("ddr_feed_qprime_f32", "ddr_feed_rows_f32")


def test_header_declares_the_entry_points():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in FUNCTIONS:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in _lib.EXPORTED
        assert hasattr(_lib.load(), name)


# ---- rows() / align(): the host lookup ---------------------------------------------------------------------------


@pytest.mark.parametrize("kind", ["int", "cat"])
def test_lookup_equals_the_dict(kind):
    rng = np.random.default_rng(11)
    store = F.ids_of(kind, rng.permutation(np.arange(1000, 1400))[:300])  # unsorted; 100 of the 400 ids absent
    batch = F.ids_of(kind, rng.integers(990, 1410, 500))  # present, absent and repeated ids
    batch += [store[3], store[3], store[0], store[-1]]  # a duplicated batch id is looked up twice
    index = RowIndex(np.array(store))
    got = index.lookup(np.array(batch))
    want = F.dict_rows(store, batch)
    assert got.dtype == np.int32 and got.shape == (len(batch),)
    np.testing.assert_array_equal(got, want)
    assert (want == -1).any() and (want >= 0).any() and got[-4] == got[-3] == 3
    # python lists, as a zarr group's id array gives once decoded; and the whole domain at once (align)
    np.testing.assert_array_equal(RowIndex(store).lookup(batch), want)
    domain = F.ids_of(kind, np.arange(990, 1410))
    np.testing.assert_array_equal(index.lookup(domain), F.dict_rows(store, domain))


@pytest.mark.parametrize("kind", ["int", "cat"])
def test_lookup_empty_store_and_empty_batch(kind):
    store = F.ids_of(kind, [5, 9, 2])
    empty = np.array([], dtype=np.asarray(store).dtype)
    assert RowIndex(store).lookup(empty).tolist() == []
    assert RowIndex(store).lookup(empty).dtype == np.int32
    assert RowIndex(empty).lookup(store).tolist() == [-1, -1, -1]
    assert RowIndex(empty).lookup(empty).tolist() == []
    assert len(RowIndex(empty)) == 0 and len(RowIndex(store)) == 3


def test_lookup_details():
    # an id carried by two rows: the dict keeps the last row
    assert RowIndex([7, 3, 7, 1]).lookup([7, 1, 3, 4]).tolist() == F.dict_rows([7, 3, 7, 1], [7, 1, 3, 4]).tolist()
    assert RowIndex([7, 3, 7, 1]).lookup([7]).tolist() == [2]
    # numeric order is not text order
    store = [f"cat-{i}" for i in (10, 9, 100, 1)]
    assert RowIndex(store).lookup(["cat-1", "cat-9", "cat-10", "cat-100", "cat-99"]).tolist() == [3, 1, 0, 2, -1]
    assert RowIndex(np.array([2**40, 5, -3])).lookup(np.array([-3, 2**40, 6])).tolist() == [2, 0, -1]
    with pytest.raises(ValueError, match="1-D"):
        RowIndex(np.zeros((2, 2), np.int64))
    with pytest.raises(TypeError):
        RowIndex(np.array([1.5, 2.5]))
    with pytest.raises(TypeError):
        RowIndex([1, 2, 3]).lookup(["cat-1"])


def test_gauge_ids_are_zero_filled_to_eight_digits():
    ids = [1234567, "01234567", 12345678, "123", 123456789]
    want = [str(g).zfill(8) for g in ids]  # readers.py:558
    assert pad_gage_ids(ids).tolist() == want == ["01234567", "01234567", "12345678", "00000123", "123456789"]
    assert pad_gage_ids(np.array([1234567, 42])).tolist() == ["01234567", "00000042"]
    index = RowIndex(pad_gage_ids(["01234567", "00000042", "12345678"]))
    assert index.lookup(pad_gage_ids([42, 1234567, "12345678", 7])).tolist() == [1, 0, 2, -1]


# ---- window arithmetic -------------------------------------------------------------------------------------------


def test_daily_window_with_a_store_that_starts_after_the_origin():
    offset = int((np.datetime64("1981-10-01") - np.datetime64("1980-01-01")).astype(int))  # (Timestamp - origin).days
    for first, rho in ((offset, 4), (offset + 700, 90), (offset + 3, 2)):
        dates = F.dates_like(first, rho)
        d0, n_days, T = daily_window(dates, "1981/10/01")
        want = dates.numerical_time_range - offset  # readers.py:497
        assert (d0, n_days) == (int(want[0]), len(want)) and T == (rho - 1) * 24 == (len(want) - 1) * 24
    assert daily_window(F.dates_like(10, 5), "1980/01/01")[0] == 10
    assert daily_window(F.dates_like(10, 5), np.datetime64("1980-01-03"))[0] == 8
    assert daily_window(F.dates_like(3, 5), "1980/01/10")[0] == -6  # before the store: feed_plan refuses it
    with pytest.raises(ValueError, match="contiguous"):
        daily_window(SimpleNamespace(numerical_time_range=np.array([3, 4, 6]), batch_hourly_time_range=range(48)),
                     "1980/01/01")
    with pytest.raises(ValueError, match="empty"):
        daily_window(SimpleNamespace(numerical_time_range=np.array([]), batch_hourly_time_range=[]), "1980/01/01")


def test_hourly_window():
    dates = F.dates_like(400, 4)
    start = np.datetime64("1980-10-01T00:00:00")
    # readers.py:491-494: ((hourly_timestamps - store_start).total_seconds() // 3600).astype(int)
    want = ((dates.batch_hourly_time_range - start.astype("datetime64[ns]")) // np.timedelta64(3600, "s")).astype(int)
    assert hourly_window(dates, "1980/10/01") == (int(want[0]), 72) and want[-1] - want[0] == 71
    assert hourly_window(dates, "1980-10-01 06:00:00")[0] == int(want[0]) - 6
    assert hourly_window(dates, "1980/01/01") == (400 * 24, 72)
    gap = SimpleNamespace(batch_hourly_time_range=dates.batch_hourly_time_range[[0, 1, 3]])
    with pytest.raises(ValueError, match="contiguous"):
        hourly_window(gap, "1980/01/01")


def _batch(ids, first, rho):
    return SimpleNamespace(divide_ids=np.asarray(ids), dates=F.dates_like(first, rho))


def test_feed_plan_windows_and_refusals():
    index = RowIndex([11, 12, 13, 14])
    rows, t0, n_cols, repeat, T = feed_plan(index, "1980/01/11", False, 100, _batch([14, 99, 11], 20, 5))
    assert rows.tolist() == [3, -1, 0] and (t0, n_cols, repeat, T) == (10, 4, 24, 96)  # the last day is not read
    rows, t0, n_cols, repeat, T = feed_plan(index, "1980/01/11", True, 2400, _batch([12], 20, 5))
    assert rows.tolist() == [1] and (t0, n_cols, repeat, T) == (240, 96, 1, 96)
    # the window's last day must lie inside the store although it is never read (readers.py:503-506)
    assert feed_plan(index, "1980/01/11", False, 15, _batch([12], 20, 5))[1] == 10
    for first, n_store, hourly in ((20, 14, False), (9, 100, False), (20, 240 + 95, True), (9, 2400, True)):
        with pytest.raises(ValueError, match=r"the store holds \[0, ") as e:
            feed_plan(index, "1980/01/11", hourly, n_store, _batch([12], first, 5))
        assert "the batch asks for" in str(e.value)  # (both ranges are named)
    with pytest.raises(AssertionError, match="No valid divide IDs found in this batch. Throwing error"):
        feed_plan(index, "1980/01/11", False, 100, _batch([1, 2, 3], 20, 5))
    with pytest.raises(AssertionError, match="No valid divide IDs"):
        feed_plan(index, "1980/01/11", False, 100, _batch([], 20, 5))


# ---- the stores' argument checks ---------------------------------------------------------------------------------


def test_python_argument_errors():
    """dtype, rank and id count raise before a device is touched; a host store raises RuntimeError."""
    ids = [3, 4, 5]
    for cls, name in ((StreamflowStore, "qr"), (ObservationStore, "streamflow")):
        with pytest.raises(ValueError, match="float32"):
            cls(np.zeros((3, 10), np.float64), ids)
        with pytest.raises(ValueError, match="float32"):
            cls(torch.zeros(3, 10, dtype=torch.float16), ids)
        for shape in ((30,), (3, 2, 5)):
            with pytest.raises(ValueError, match="2-D"):
                cls(np.zeros(shape, np.float32), ids)
        with pytest.raises(ValueError, match="3 ids"):
            cls(np.zeros((4, 10), np.float32), ids)
        with pytest.raises(TypeError):
            cls([[0.0] * 10] * 3, ids)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            cls(torch.zeros(3, 10), ids)  # a host tensor
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            cls(np.zeros((3, 10), np.float32), ids, device="cpu")
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            cls(torch.zeros(3, 10), ids, device="cpu")


# ---- the C ABI's refusals (no device needed: every call is refused before a launch) --------------------------------


def test_feed_qprime_refusals():
    lib = _lib.load()
    p = 4096  # (never dereferenced)

    def run(store=p, stride=100, n_rows=8, T=100, rows=p, N=5, t0=10, n_cols=4, repeat=1, n_out=4, out=p, valid=p):
        return lib.ddr_feed_qprime_f32(store, stride, n_rows, T, rows, N, t0, n_cols, repeat, n_out, 0.001, out, valid,
                                       None)

    for kw in ({"stride": -1}, {"n_rows": -1}, {"T": -1}, {"N": -1}, {"n_cols": -1}, {"n_out": -1, "n_cols": 0}):
        assert run(**kw) == _lib.DDR_ERR_ARG and b"negative" in lib.ddr_last_error(), kw
    assert run(stride=99) == _lib.DDR_ERR_ARG and b"row_stride" in lib.ddr_last_error()
    assert run(n_rows=2**31) == _lib.DDR_ERR_ARG and b"32-bit" in lib.ddr_last_error()
    for kw in ({"t0": -1}, {"t0": 97}, {"t0": 101, "n_cols": 0, "n_out": 0}, {"n_cols": 91, "n_out": 91}):
        assert run(**kw) == _lib.DDR_ERR_ARG and b"leaves the store" in lib.ddr_last_error(), kw
    for repeat in (0, -24):
        assert run(repeat=repeat) == _lib.DDR_ERR_ARG and b"repeat" in lib.ddr_last_error()
    for kw in ({"n_out": 5}, {"repeat": 24, "n_out": 72}, {"repeat": 24, "n_out": 97}, {"n_cols": 0}):
        assert run(**kw) == _lib.DDR_ERR_ARG and b"ceil" in lib.ddr_last_error(), kw
    for kw in ({"store": None}, {"rows": None}, {"out": None}, {"valid": None}):
        assert run(**kw) == _lib.DDR_ERR_ARG and b"null" in lib.ddr_last_error(), kw
    assert run(N=0, store=None, rows=None, out=None, valid=None) == _lib.DDR_OK  # no reaches: a no-op
    assert run(N=0, repeat=0) == _lib.DDR_ERR_ARG  # (still checked)


def test_feed_rows_refusals():
    lib = _lib.load()
    p = 4096

    def run(store=p, stride=100, n_rows=8, T=100, rows=p, G=5, t0=10, n_cols=6, trim=1, out=p, out_stride=4, nan=p):
        return lib.ddr_feed_rows_f32(store, stride, n_rows, T, rows, G, t0, n_cols, trim, out, out_stride, nan, None)

    for kw in ({"stride": -1}, {"n_rows": -1}, {"T": -1}, {"G": -1}, {"n_cols": -1}, {"trim": -1}, {"out_stride": -1}):
        assert run(**kw) == _lib.DDR_ERR_ARG and b"negative" in lib.ddr_last_error(), kw
    assert run(stride=99) == _lib.DDR_ERR_ARG and b"row_stride" in lib.ddr_last_error()
    for kw in ({"t0": -1}, {"t0": 95}, {"n_cols": 91, "out_stride": 89}):
        assert run(**kw) == _lib.DDR_ERR_ARG and b"leaves the store" in lib.ddr_last_error(), kw
    assert run(n_cols=1) == _lib.DDR_ERR_ARG and b"each end" in lib.ddr_last_error()
    assert run(out_stride=3) == _lib.DDR_ERR_ARG and b"out_stride" in lib.ddr_last_error()
    for kw in ({"store": None}, {"rows": None}, {"out": None}, {"nan": None}):
        assert run(**kw) == _lib.DDR_ERR_ARG and b"null" in lib.ddr_last_error(), kw
    assert run(G=0, store=None, rows=None, out=None, nan=None) == _lib.DDR_OK
