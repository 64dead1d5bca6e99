"""The summed-Q' baseline without a GPU: the C ABI's declarations and refusals, members_from_ids against the
reference's per-gauge np.isin, the Python argument checks, and the summedq.npz fixture's coverage."""

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from conftest import load_golden
from ddr_amd import _lib
from ddr_amd.validation import SummedQPrime, members_from_ids, summed_q_prime_metrics

HEADER = Path(__file__).resolve().parents[1] / "include" / "ddr_mc.h"
FUNCTIONS = ("ddr_summedq_plan_create", "ddr_summedq_plan_destroy", "ddr_summedq_scratch_bytes", "ddr_summedq_f32")

HOURLY_T = (24, 25, 47, 24 * 63, 24 * 64 + 5, 24 * 65)
DAILY_D = (1, 3, 63, 64, 65, 255, 256, 257, 1031)
LIST_LENGTHS = (0, 1, 7, 8, 9, 16, 17, 27)


def test_header_declares_the_entry_points():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in FUNCTIONS:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in _lib.EXPORTED
    assert hasattr(_lib.load(), "ddr_summedq_f32")


def make_plan(lib, lists, chunk=4096):
    off = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(m) for m in lists], out=off[1:])
    idx = np.array([i for m in lists for i in m], np.int32)
    plan = C.c_void_p()
    code = lib.ddr_summedq_plan_create(len(lists), off.ctypes.data, idx.ctypes.data if idx.size else None, chunk, None,
                                       C.byref(plan))
    return code, plan


def test_plan_create_refusals():
    lib = _lib.load()
    plan = C.c_void_p()
    off = np.array([0, 2, 3], np.int64)
    idx = np.array([4, 1, 7], np.int32)

    def create(G, off_, idx_, chunk, out=plan):
        return lib.ddr_summedq_plan_create(G, None if off_ is None else off_.ctypes.data,
                                           None if idx_ is None else idx_.ctypes.data, chunk,
                                           None, None if out is None else C.byref(out))

    assert create(-1, off, idx, 8) == _lib.DDR_ERR_ARG and b"negative" in lib.ddr_last_error()
    for chunk in (0, -5):
        assert create(2, off, idx, chunk) == _lib.DDR_ERR_ARG and b"chunk" in lib.ddr_last_error()
    assert create(2, None, idx, 8) == _lib.DDR_ERR_ARG and b"null" in lib.ddr_last_error()
    assert create(2, off, None, 8) == _lib.DDR_ERR_ARG and b"null" in lib.ddr_last_error()
    assert create(2, off, idx, 8, out=None) == _lib.DDR_ERR_ARG and b"null" in lib.ddr_last_error()
    for bad in ([0, 3, 2], [1, 2, 3], [0, -1, 3]):
        assert create(2, np.array(bad, np.int64), idx, 8) == _lib.DDR_ERR_ARG
        assert b"monotone" in lib.ddr_last_error()
    assert create(2, off, np.array([4, -1, 7], np.int32), 8) == _lib.DDR_ERR_ARG
    assert b"negative index" in lib.ddr_last_error()
    assert not plan.value  # (a refused call leaves no plan behind)


def test_run_refusals():
    """ddr_summedq_f32 checks everything before any launch: with no device the plan still carries the lists."""
    lib = _lib.load()
    code, plan = make_plan(lib, [[4, 1], [], [7] * 20], chunk=8)  # the third list is cut into three pieces
    assert code == _lib.DDR_OK and plan.value
    try:
        assert lib.ddr_summedq_scratch_bytes(plan, 10) == 3 * 10 * 8
        assert lib.ddr_summedq_scratch_bytes(plan, 0) == 0
        assert lib.ddr_summedq_scratch_bytes(plan, -1) == -1
        assert lib.ddr_summedq_scratch_bytes(None, 10) == -1
        p = 4096  # (never dereferenced: every call below is refused)
        big = 1 << 20

        def run(n_rows=8, stride=48, T=48, rho=24, out=p, out_stride=2, scratch=p, nbytes=big, qr=p, plan_=plan):
            return lib.ddr_summedq_f32(plan_, qr, n_rows, stride, T, rho, out, out_stride, scratch, nbytes, None)

        for kw in ({"n_rows": -1}, {"stride": -1}, {"T": -1}, {"out_stride": -1}, {"nbytes": -1}):
            assert run(**kw) == _lib.DDR_ERR_ARG and b"negative" in lib.ddr_last_error(), kw
        for rho in (0, 2, 12, 25, -24):
            assert run(rho=rho) == _lib.DDR_ERR_ARG and b"1 or 24" in lib.ddr_last_error(), rho
        assert run(T=23, stride=23) == _lib.DDR_ERR_ARG and b"T < rho" in lib.ddr_last_error()
        assert run(T=0, stride=0, rho=1) == _lib.DDR_ERR_ARG and b"T < rho" in lib.ddr_last_error()
        assert run(stride=47) == _lib.DDR_ERR_ARG and b"row_stride" in lib.ddr_last_error()
        assert run(out_stride=1) == _lib.DDR_ERR_ARG and b"out_stride" in lib.ddr_last_error()
        for n_rows in (7, 0):
            assert run(n_rows=n_rows) == _lib.DDR_ERR_ARG and b"largest" in lib.ddr_last_error()
        assert run(nbytes=3 * 2 * 8 - 1) == _lib.DDR_ERR_ARG and b"scratch_bytes" in lib.ddr_last_error()
        for kw in ({"qr": None}, {"out": None}, {"scratch": None}, {"plan_": None}):
            assert run(**kw) == _lib.DDR_ERR_ARG and b"null" in lib.ddr_last_error(), kw
    finally:
        assert lib.ddr_summedq_plan_destroy(plan) == _lib.DDR_OK
    assert lib.ddr_summedq_plan_destroy(None) == _lib.DDR_OK


def test_zero_gauges_is_a_noop():
    lib = _lib.load()
    code, plan = make_plan(lib, [])
    assert code == _lib.DDR_OK
    assert lib.ddr_summedq_scratch_bytes(plan, 100) == 0
    assert lib.ddr_summedq_f32(plan, None, 0, 24, 24, 24, None, 1, None, 0, None) == _lib.DDR_OK
    assert lib.ddr_summedq_f32(plan, None, 0, 24, 24, 7, None, 1, None, 0, None) == _lib.DDR_ERR_ARG
    lib.ddr_summedq_plan_destroy(plan)


def isin_lists(row_ids, gauge_ids):
    """The reference's formulation (scripts/summed_q_prime.py:258), one isin per gauge."""
    return [np.where(np.isin(row_ids, ids))[0] for ids in gauge_ids]


@pytest.mark.parametrize("kind", ["int", "cat"])
def test_members_from_ids_equals_isin(kind):
    rng = np.random.default_rng(5)
    store = rng.permutation(np.arange(1000, 1400))[:300]  # unsorted, 100 of the 400 ids absent
    gauges = [rng.choice(np.arange(1000, 1400), size=m, replace=False) for m in (1, 5, 40, 250)]
    gauges.insert(2, np.array([], np.int64))  # an empty gauge
    gauges.append(np.setdiff1d(np.arange(1000, 1400), store)[:30])  # every id missing from the store
    gauges.append(np.array([store[3], store[3], 99999, store[0]]))  # a repeated id, an unknown one
    if kind == "cat":
        store = np.array([f"cat-{i}" for i in store])
        gauges = [np.array([f"cat-{i}" for i in ids]) for ids in gauges]
    off, idx = members_from_ids(store, gauges)
    assert off.dtype == np.int64 and idx.dtype == np.int32 and off.shape == (len(gauges) + 1,)
    assert off[0] == 0 and off[-1] == idx.size
    want = isin_lists(store, [ids if len(ids) else np.array([], store.dtype) for ids in gauges])
    for g, w in enumerate(want):
        assert np.array_equal(idx[off[g]:off[g + 1]], w), g
    assert off[3] == off[2] and off[6] == off[5]  # the empty gauge and the all-missing one
    assert 0 < off[4] - off[3] < 40  # some of that gauge's ids are absent


def test_members_from_ids_edge_cases():
    off, idx = members_from_ids(np.arange(5), [])
    assert off.tolist() == [0] and idx.size == 0
    off, idx = members_from_ids(np.arange(5), [[], []])
    assert off.tolist() == [0, 0, 0] and idx.size == 0
    off, idx = members_from_ids(np.array([7, 3, 7, 1]), [[7], [1, 3]])  # an id carried by two rows selects both
    assert off.tolist() == [0, 2, 4] and idx.tolist() == [0, 2, 1, 3]
    # python lists of strings, as a zarr group's order array gives once decoded
    off, idx = members_from_ids(["cat-3", "cat-10", "cat-1"], [["cat-1", "cat-10"], ["cat-2"]])
    assert off.tolist() == [0, 2, 2] and idx.tolist() == [1, 2]


def test_python_argument_errors():
    """dtype, rank and hours_per_step raise before the device is touched; host tensors raise RuntimeError."""
    s = SummedQPrime(np.array([0, 2, 3]), np.array([4, 1, 7]), chunk=8)
    assert s.n_gauges == 2 and s.max_index == 7 and s.scratch_bytes(10) == 0
    z = torch.zeros
    with pytest.raises(ValueError, match="float32"):
        s(z(8, 48, dtype=torch.float64))
    with pytest.raises(ValueError, match="float32"):
        s(z(8, 48, dtype=torch.float16), 1)
    for shape in ((48,), (8, 2, 24)):
        with pytest.raises(ValueError, match="2-D"):
            s(z(*shape))
    for rho in (0, 2, 12, 25, -1):
        with pytest.raises(ValueError, match="hours_per_step"):
            s(z(8, 48), rho)
    with pytest.raises(ValueError, match="one day"):
        s(z(8, 23))
    with pytest.raises(ValueError, match="rows"):
        s(z(7, 48))
    with pytest.raises(TypeError):
        s(np.zeros((8, 48), np.float32))
    with pytest.raises(RuntimeError, match="HIP device only"):
        s(z(8, 48))
    with pytest.raises(RuntimeError, match="HIP device only"):
        s(z(8, 48), 1)
    with pytest.raises(RuntimeError, match="HIP device only"):
        summed_q_prime_metrics(s, z(8, 48), z(2, 2))
    with pytest.raises(ValueError, match="off"):
        SummedQPrime(np.array([0, 2, 4]), np.array([4, 1, 7]))
    with pytest.raises(_lib.DDRError, match="monotone"):
        SummedQPrime(np.array([0, 4, 3]), np.array([4, 1, 7]))
    with pytest.raises(_lib.DDRError, match="negative index"):
        SummedQPrime(np.array([0, 2, 3]), np.array([4, -1, 7]))
    with pytest.raises(_lib.DDRError, match="chunk"):
        SummedQPrime(np.array([0, 2, 3]), np.array([4, 1, 7]), chunk=0)


def test_fixture_holds_every_case():
    d = load_golden("summedq")
    tags = set(d["cases"].tolist())
    want = {f"h{T}" for T in HOURLY_T} | {f"d{D}" for D in DAILY_D} | {"lists_d", "lists_h", "big"}
    assert want <= tags
    for tag in want:
        qr = d[str(d[f"store_{tag}"])]
        rho, T = int(d[f"rho_{tag}"]), int(d[f"T_{tag}"])
        off, idx = d[f"off_{tag}"], d[f"idx_{tag}"]
        G, D = len(off) - 1, T // rho
        assert qr.dtype == np.float32 and qr.shape[1] >= T and rho in (1, 24)
        assert off.dtype == np.int64 and idx.dtype == np.int32 and off[-1] == idx.size
        assert idx.size == 0 or (0 <= idx.min() and idx.max() < qr.shape[0])
        assert d[f"ref_{tag}"].shape == (G, D) and d[f"ref_{tag}"].dtype == np.float32
        assert d[f"model_{tag}"].shape == (G, D) and d[f"model_{tag}"].dtype == np.float64
        assert 1 <= G <= 16 and qr.shape[0] <= 9000
    for tag in (f"h{T}" for T in HOURLY_T):
        assert int(d[f"rho_{tag}"]) == 24 and int(d[f"T_{tag}"]) == int(tag[1:])
    for tag in (f"d{D}" for D in DAILY_D):
        assert int(d[f"rho_{tag}"]) == 1 and int(d[f"T_{tag}"]) == int(tag[1:])
    for tag in ("lists_d", "lists_h"):
        assert tuple(np.diff(d[f"off_{tag}"]).tolist()) == LIST_LENGTHS
    assert np.diff(d["off_big"]).tolist() == [2 * 4096 + 1] and int(d["T_big"]) == 70
    # the special rows: NaN at single hours, NaN throughout, +inf; a gauge that is all NaN on some days gives 0.0
    rows = dict(zip(d["special_names"].tolist(), d["special_rows"].tolist()))
    qr = d["qr_long"]
    nan_hours = np.isnan(qr[rows["nan_hours"]])
    assert nan_hours.any() and not nan_hours.all()
    per_day = nan_hours[: 24 * 65].reshape(65, 24).sum(axis=1)
    assert ((per_day > 0) & (per_day < 24)).any() and (per_day == 0).any()  # NaN hours inside a day; clean days
    assert np.isnan(qr[rows["all_nan"]]).all()
    assert np.isposinf(qr[rows["plus_inf"]]).any() and not np.isnan(qr[rows["plus_inf"]]).any()
    for tag in ("h1560", "d257"):
        off, idx, model = d[f"off_{tag}"], d[f"idx_{tag}"], d[f"model_{tag}"]
        assert sorted(idx[off[1]:off[2]].tolist()) == sorted([rows["nan_hours"], rows["all_nan"]])
        assert (model[1] == 0.0).any() and (model[1] > 0.0).any()
        assert np.isposinf(model[2]).any() and np.isfinite(model[2]).any()
        assert rows["nan_hours"] in idx[off[0]:off[1]] and rows["all_nan"] in idx[off[0]:off[1]]
        assert np.isfinite(model[0]).all() and (model[0] > 0).all()
    assert any(int(d[f"T_h{T}"]) % 24 for T in HOURLY_T)  # trailing hours that do not fill a day
