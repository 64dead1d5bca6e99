"""The forcing feed on the device (csrc/feed.hip) against the NumPy restatements of feed_cases.py, bitwise: tile
edges, load alignment, missing and repeated rows, the hourly expansion, 64-bit row offsets, the observation windows,
the router fed both ways, and the reference's drop-in call."""

from types import SimpleNamespace

import numpy as np
import pytest
import torch

import feed_cases as F
from ddr_amd import synthetic
from ddr_amd.graph import RiverGraph
from ddr_amd.io import ObservationStore, StreamflowStore
from ddr_amd.ops import route
from oracle import mc_oracle as O

pytestmark = pytest.mark.gpu

N_ROWS, T_STORE = 300, 1031
TILE_N = (1, 63, 64, 65, 129, 257)
TILE_COLS = (1, 2, 63, 64, 65, 130)


@pytest.fixture(scope="module")
def qr():
    q = F.lognormal_store(N_ROWS, T_STORE, seed=0)
    q.setflags(write=False)
    return q


@pytest.fixture(scope="module")
def flow(cuda, qr):
    return StreamflowStore(qr, np.arange(N_ROWS), device=cuda)


def dev_rows(rows, cuda):
    return torch.from_numpy(np.asarray(rows, np.int32)).to(cuda)


def check_daily(store, qr, rows, t0, n_cols, cuda):
    qd, valid = store.daily(dev_rows(rows, cuda), t0, n_cols)
    want, ok = F.expected_gather(qr, rows, t0, n_cols)
    assert qd.dtype == torch.float32 and valid.dtype == torch.bool and qd.is_contiguous()
    assert tuple(qd.shape) == (n_cols, len(rows)) and tuple(valid.shape) == (len(rows),)
    assert F.same_bits(qd.cpu().numpy(), want), (len(rows), t0, n_cols)
    np.testing.assert_array_equal(valid.cpu().numpy(), ok)


def hours_namespace(ids, first_day: int, T: int) -> SimpleNamespace:
    """A batch of ``T`` hourly steps from day ``first_day``: the days they touch and the boundary day after."""
    dates = F.dates_like(first_day, -(-T // 24) + 1)
    dates.batch_hourly_time_range = dates.batch_hourly_time_range[:T]
    return SimpleNamespace(divide_ids=np.asarray(ids), dates=dates)


@pytest.mark.parametrize("N", TILE_N)
def test_tile_edges(cuda, qr, flow, N):
    rows = F.batch_rows(N_ROWS, N, seed=N)
    if N > 4:
        assert set(F.SPECIAL.values()) <= set(rows.tolist())
    for n_cols in TILE_COLS:
        for t0 in (0, 7):
            check_daily(flow, qr, rows, t0, n_cols, cuda)


@pytest.mark.parametrize("stride", [1031, 1032, 1036, "1036+1"])
def test_alignment(cuda, qr, stride):
    """16-byte loads (aligned base, stride a multiple of 4) and 4-byte loads (odd stride, or a base one element off),
    for every residue of t0; the window's end at the store's end reads the row's last, partial quad."""
    width, shift = (1036, 1) if stride == "1036+1" else (stride, 0)
    wide = torch.full((N_ROWS, width), float("nan"), device=cuda)
    view = wide[:, shift:shift + T_STORE]
    view.copy_(torch.from_numpy(qr))
    assert view.stride() == (width, 1) and (view.data_ptr() % 16 == 0) == (shift == 0)
    store = StreamflowStore(view, np.arange(N_ROWS))
    assert store.qr.data_ptr() == view.data_ptr()  # (kept, not copied)
    rows = F.batch_rows(N_ROWS, 70, seed=3)
    for t0 in (0, 1, 2, 3, 5):
        for n_cols in (1, 64, 130, T_STORE - t0, T_STORE - t0 - 1):
            check_daily(store, qr, rows, t0, n_cols, cuda)
    check_daily(store, qr, rows, T_STORE - 1, 1, cuda)
    check_daily(store, qr, rows, T_STORE, 0, cuda)


def test_missing_and_repeated_rows(cuda, qr, flow):
    base = F.batch_rows(N_ROWS, 129, seed=8)
    cases = {}
    for name, where in (("first-of-tile", [0, 64, 128]), ("last-of-tile", [63, 127])):
        r = base.copy()
        r[where] = -1
        cases[name] = r
    r = np.full(129, -1, np.int32)
    r[77] = 41
    cases["all-missing-but-one"] = r
    cases["all-missing"] = np.full(65, -1, np.int32)
    r = base.copy()
    r[[1, 2, 3, 64, 100, 128]] = 17
    cases["one-row-for-several-reaches"] = r
    r = base.copy()
    r[[0, 5, 63, 64]] = [N_ROWS, -5, N_ROWS + 1000, np.iinfo(np.int32).min]
    r[70] = np.iinfo(np.int32).max
    cases["out-of-range-indices"] = r
    for name, rows in cases.items():
        for t0, n_cols in ((0, 1), (3, 65), (130, 90)):
            check_daily(flow, qr, rows, t0, n_cols, cuda)
    want, ok = F.expected_gather(qr, cases["out-of-range-indices"], 3, 65)
    assert not ok[[0, 5, 63, 64, 70]].any() and ok.sum() == 129 - 5
    assert (want[:, ~ok] == F.FILL).all()


@pytest.mark.parametrize("T", [24, 25, 47, 72, 24 * 64 + 5])
def test_hourly_expansion_of_a_daily_store(cuda, qr, T):
    first = 30 + 5  # the store starts 30 days after the origin
    store = StreamflowStore(qr, np.arange(N_ROWS), start="1980/01/31", device=cuda)
    for N in (65, 130):
        ids = F.batch_rows(N_ROWS + 20, N, seed=T + N)  # ids N_ROWS .. N_ROWS + 19 are not in the store
        out = store(routing_dataclass=hours_namespace(ids, first, T), device=cuda, dtype=torch.float32)
        rows = np.where(ids < N_ROWS, ids, -1)
        n_cols = -(-T // 24)
        want = np.full((T, N), F.FILL, np.float32)
        want[:, rows >= 0] = np.repeat(qr[rows[rows >= 0], 5:5 + n_cols], 24, axis=1)[:, :T].T
        assert tuple(out.shape) == (T, N) and F.same_bits(out.cpu().numpy(), want), (T, N)
        assert F.same_bits(want, F.expected_gather(qr, rows, 5, n_cols, 24, T)[0])


def test_training_shape_and_hourly_store(cuda, qr):
    """rho = 4: T = (rho - 1) * 24 from a daily store (its last day is not read), and the same batch from an hourly
    store (repeat = 1), against readers.py:477-531."""
    rho, first = 4, 40
    store_ids = F.ids_of("cat", np.random.default_rng(2).permutation(N_ROWS) + 1000)
    batch_ids = F.ids_of("cat", np.random.default_rng(3).integers(990, 1000 + N_ROWS + 10, 131))
    batch = SimpleNamespace(divide_ids=np.array(batch_ids), dates=F.dates_like(first, rho))
    T = (rho - 1) * 24
    assert len(batch.dates.batch_hourly_time_range) == T

    daily = StreamflowStore(qr, store_ids, start="1980/01/11", is_hourly=False, device=cuda)
    time_idx = batch.dates.numerical_time_range - 10  # readers.py:497
    want = F.streamflow_reader(qr, store_ids, batch_ids, time_idx, False, T)
    assert (want[:, [b not in set(store_ids) for b in batch_ids]] == F.FILL).all()
    got = daily(routing_dataclass=batch, device=cuda, dtype=torch.float32)
    assert F.same_bits(got.cpu().numpy(), want)
    q, valid = daily.hourly(daily.rows(batch_ids), int(time_idx[0]), T)  # the same without the host lookups
    assert F.same_bits(q.cpu().numpy(), want)
    np.testing.assert_array_equal(valid.cpu().numpy(), F.dict_rows(store_ids, batch_ids) >= 0)
    poisoned = qr.copy()
    poisoned[:, time_idx[-1]] = 12345.0  # the window's last day is never read
    again = StreamflowStore(poisoned, store_ids, start="1980/01/11", device=cuda)(routing_dataclass=batch)
    assert F.same_bits(again.cpu().numpy(), want)

    hourly = StreamflowStore(qr, store_ids, start="1980/01/11", is_hourly=True, device=cuda)  # 1031 hours from day 10
    batch_h = SimpleNamespace(divide_ids=np.array(batch_ids), dates=F.dates_like(11, rho))
    time_idx = 24 + np.arange(T)  # readers.py:491-494: whole hours since the store's start
    want = F.streamflow_reader(qr, store_ids, batch_ids, time_idx, True, T)
    got = hourly(routing_dataclass=batch_h, device=cuda, dtype=torch.float32)
    assert F.same_bits(got.cpu().numpy(), want)
    t0, n_cols, T_ = hourly.window_of(batch_h.dates)
    assert (t0, n_cols, T_) == (24, T, T) and hourly.hours_per_column == 1 and daily.hours_per_column == 24
    qd, valid = hourly.daily(hourly.rows(batch_ids), t0, n_cols)
    assert F.same_bits(qd.cpu().numpy(), want)

    # the batch collated on the device: rows from the aligned domain, no host lookup
    domain = F.ids_of("cat", np.arange(990, 1000 + N_ROWS + 10))
    aligned = daily.align(domain)
    active = torch.from_numpy(np.array([int(b[4:]) - 990 for b in batch_ids], np.int32)).to(cuda)
    rows = aligned[active]  # (int32 indices, as DeviceBatch.active holds them)
    assert rows.dtype == torch.int32 and torch.equal(rows, daily.rows(batch_ids))
    np.testing.assert_array_equal(rows.cpu().numpy(), F.dict_rows(store_ids, batch_ids))

    with pytest.raises(AssertionError, match="No valid divide IDs found in this batch. Throwing error"):
        daily(routing_dataclass=SimpleNamespace(divide_ids=np.array(["cat-1", "cat-2"]), dates=batch.dates))
    for first_day in (9, 10 + T_STORE - rho + 1):
        with pytest.raises(ValueError, match="the store holds"):
            daily(routing_dataclass=SimpleNamespace(divide_ids=batch.divide_ids, dates=F.dates_like(first_day, rho)))
    assert daily(routing_dataclass=SimpleNamespace(divide_ids=batch.divide_ids,
                                                   dates=F.dates_like(10 + T_STORE - rho, rho))).shape == (T, 131)
    with pytest.raises(ValueError, match="leaves the store"):
        daily.daily(rows, T_STORE - 2, 3)
    with pytest.raises(ValueError, match="int32"):
        daily.daily(rows.long(), 0, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        daily.daily(rows.cpu(), 0, 3)


def test_row_offsets_beyond_32_bits(cuda):
    """A 4-row store with a row stride of 2^30 elements: rows 2 and 3 start beyond 2^32 bytes, row 3 beyond 2^31
    elements.  Only the 4 x 8 cells that are read are written."""
    if torch.cuda.mem_get_info()[0] < 16 * 2**30:
        pytest.skip("needs 16 GiB of free device memory")
    stride = 2**30
    buf = torch.empty(3 * stride + 64, device=cuda, dtype=torch.float32)
    cells = np.random.default_rng(4).lognormal(0.0, 1.0, (4, 8)).astype(np.float32)
    rows = np.array([3, 0, 2, -1, 1, 3, 4], np.int32)
    for shift in (0, 1):  # 16-byte loads, and 4-byte loads from a base one element off
        view = buf.as_strided((4, 8), (stride, 1), shift)
        view.copy_(torch.from_numpy(cells))
        store = StreamflowStore(view, np.arange(4))
        assert store.qr.data_ptr() == buf.data_ptr() + 4 * shift
        for t0, n in ((0, 8), (1, 6), (5, 3)):
            check_daily(store, cells, rows, t0, n, cuda)
        out = store(routing_dataclass=hours_namespace([3, 9, 2, 0, 1], 2, 49))
        assert F.same_bits(out.cpu().numpy(), F.expected_gather(cells, [3, -1, 2, 0, 1], 2, 3, 24, 49)[0])
        obs = ObservationStore(view, np.arange(4))
        target, has_nan = obs.window(dev_rows([3, 2, -1, 0], cuda), 1, 6)
        want, flag = F.expected_observations(cells, [3, 2, -1, 0], 1, 6)
        assert F.same_bits(target.cpu().numpy(), want) and has_nan.cpu().tolist() == flag.tolist()
    del buf, view, store, obs


@pytest.mark.parametrize("n_days", [3, 4, 65, 257])
def test_observation_windows(cuda, n_days):
    day0, n_gauges, T = 5, 70, 300
    rng = np.random.default_rng(n_days)
    obs_np = rng.lognormal(1.0, 1.0, (n_gauges, T)).astype(np.float32)
    last = day0 + n_days - 1
    obs_np[0, day0] = np.nan            # only the first day, which the target drops
    obs_np[1, last] = np.nan            # only the last day
    obs_np[2] = np.nan                  # throughout
    obs_np[4, [day0 - 1, last + 1]] = np.nan  # just outside the window: a clean row (3 is clean too)
    obs_np[5, day0 + n_days // 2] = np.nan
    obs_np[6].view(np.uint32)[day0 + 1] = 0x7FA00001  # a signalling NaN with a payload, inside the target
    gage_ids = [str(1000 + g) if g % 2 else 1000 + g for g in range(n_gauges)]  # keyed as "00001000" ...
    store = ObservationStore(obs_np, gage_ids, start="1980/01/01", device=cuda)
    for G in (1, 3, 64, 65):
        pick = ([0, 1, 2, 3, 4, 5, 6] + rng.integers(0, n_gauges, 65).tolist())[:G] if G > 3 else [1, 0, 3][:G]
        batch = [f"{1000 + g:08d}" if k % 2 else 1000 + g for k, g in enumerate(pick)]
        if G >= 3:
            batch[2] = "99999999"  # unknown
        rows = store.rows(batch)
        rows_np = rows.cpu().numpy()
        want_rows = F.dict_rows([str(g).zfill(8) for g in gage_ids], [str(b).zfill(8) for b in batch])
        np.testing.assert_array_equal(rows_np, want_rows)
        target, has_nan = store.window(rows, day0, n_days)
        want, flag = F.expected_observations(obs_np, rows_np, day0, n_days)
        assert target.dtype == torch.float32 and has_nan.dtype == torch.bool
        assert tuple(target.shape) == (G, n_days - 2) and tuple(has_nan.shape) == (G,)
        assert F.same_bits(target.cpu().numpy(), want), (G, n_days)
        np.testing.assert_array_equal(has_nan.cpu().numpy(), flag)
    # what the cases are there for
    rows = store.rows([1000, 1001, 1002, 1003, 1004, "77"])
    target, has_nan = store.window(rows, day0, n_days)
    assert has_nan.cpu().tolist() == [True, True, True, False, False, True]
    t = target.cpu().numpy()
    assert not np.isnan(t[[0, 1, 3, 4]]).any() and np.isnan(t[[2, 5]]).all()
    assert store.window_of(F.dates_like(day0, n_days)) == (day0, n_days)
    keep = ~has_nan  # the caller's filter (train.py:87-92)
    assert tuple(target[keep].shape) == (2, n_days - 2)
    with pytest.raises(ValueError, match="shorter"):
        store.window(rows, day0, 1)
    with pytest.raises(ValueError, match="leaves the store"):
        store.window(rows, T - 2, 3)


def test_into_the_router(cuda):
    """The daily window with its mask, routed with q'[t / 24] in the kernel, and the drop-in hourly tensor routed as
    is: the same runoff, final discharge and parameter gradients, bit for bit."""
    rho, first, n_store_days = 4, 3, 12
    net = synthetic.random_binary_tree(130, seed=5)
    T = (rho - 1) * 24
    at = synthetic.reach_attributes(net.n, 5)
    u = synthetic.unit_parameters(net.n, 5)
    rng = np.random.default_rng(5)
    missing = rng.choice(net.n, size=7, replace=False)
    store_ids = np.setdiff1d(np.arange(net.n), missing)[rng.permutation(net.n - 7)]
    qstore = synthetic.lateral_inflow(net.n, n_store_days, 6).T[store_ids]  # (divides, days)
    qstore = np.ascontiguousarray(qstore, np.float32)
    fs = rng.uniform(0.5, 1.5, net.n).astype(np.float32)
    batch = SimpleNamespace(divide_ids=np.arange(net.n), dates=F.dates_like(first, rho))
    flow = StreamflowStore(qstore, store_ids, device=cuda)
    d0, n_cols, T_ = flow.window_of(batch.dates)
    assert (d0, n_cols, T_) == (first, rho - 1, T)
    rows = flow.rows(batch.divide_ids)
    assert int((rows < 0).sum()) == 7

    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(cuda)  # noqa: E731
    ranges = {"n": [0.015, 0.25], "q_spatial": [0.0, 1.0], "p_spatial": [1.0, 200.0]}
    phys = (O.denormalize(u["n"], ranges["n"]), O.denormalize(u["q_spatial"], ranges["q_spatial"]),
            O.denormalize(u["p_spatial"], ranges["p_spatial"], True))
    slope = np.maximum(at.slope, np.float32(1e-3))
    g = RiverGraph(net.n, net.rows, net.cols)
    W = tt(rng.uniform(0, 1, (net.n, T)))
    outs = []
    for fed in ("daily", "drop-in"):
        n, q, p = (tt(v).requires_grad_(True) for v in phys)
        if fed == "daily":
            qd, valid = flow.daily(rows, d0, 3)
            kw = dict(qprime_hours=24, steps=T, qprime_valid=valid)
        else:
            qd, kw = flow(routing_dataclass=batch, device=cuda, dtype=torch.float32), {}
            assert tuple(qd.shape) == (T, net.n)
        runoff, q_last, _, _ = route(g, qd, n, q, p, tt(at.length), tt(slope), tt(at.x), flow_scale=tt(fs),
                                     math="exact", **kw)
        runoff.backward(W)
        outs.append([t.detach().cpu().numpy() for t in (runoff, q_last, n.grad, q.grad, p.grad)])
    for name, a, b in zip(("runoff", "q_last", "grad n", "grad q", "grad p"), *outs):
        assert np.isfinite(a).all() and np.abs(a).max() > 0, name
        assert F.same_bits(a, b), name
