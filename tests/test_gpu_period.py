"""Whole-period inference on the device (ddr_amd/inference.py, csrc/period.hip): the reference's chunked ``ddr route`` /
``ddr test`` loop with only the daily series leaving the kernels.

Bars: daily discharge against the reference's own loop (tests/golden/period.npz) 1e-4 max-rel, the project's bar for
routed discharge against reference goldens (tests/test_gpu_state.py); against the same loop composed from the CPU
oracle 1e-6, the bar for pooled means (tests/test_gpu_objectives.py).  Everything else is bitwise: a finished day is one
sequential pass over its 24 hours, whatever the chunking.
"""

import ctypes as C

import numpy as np
import pytest
import torch

from conftest import maxrel
from ddr_amd import _lib
from ddr_amd.graph import RiverGraph
from ddr_amd.inference import PeriodRouter, period_chunks
from ddr_amd.io import ObservationStore, StreamflowStore
from ddr_amd.ops import GaugeMap, RouteConsts, mc_route, register_graph, route
from ddr_amd.validation.metrics import METRIC_NAMES, Metrics
from period_helpers import CHUNK_DAYS, MODES, TAUS, oracle_period, period_case, pool_sequential

pytestmark = pytest.mark.gpu

PARTITIONS = [None, {"max_block_reaches": 16, "target_blocks": 1 << 20}]
CONSTS = RouteConsts(discharge_lb=1e-4, velocity_lb=0.01, depth_lb=0.01, bottom_width_lb=0.01)


class Setup:
    """The period.npz case on the device in one precision and partition."""

    def __init__(self, dev, dtype=torch.float32, gkw=None):
        case, store, outflow, d = period_case()
        self.case, self.store, self.outflow, self.golden = case, store, outflow, d
        self.dev, self.dtype, self.n_days = dev, dtype, store.shape[0]
        self.tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype)  # noqa: E731
        n, q, p, slope = case.physical()
        self.n, self.q, self.p = self.tt(n), self.tt(q), self.tt(p)
        self.length, self.slope, self.x = self.tt(case.length), self.tt(slope), self.tt(case.x)
        self.daily_q = self.tt(store)
        self.graph = RiverGraph(case.n, case.rows, case.cols, **(gkw or {}))
        self.gauges = GaugeMap.build(outflow, case.n, dev)

    def router(self, B, tau, mode):
        return PeriodRouter(self.graph, self.length, self.slope, self.x, gauges=self.gauges if mode == "gauge" else None,
                            consts=CONSTS, tau=tau, chunk_days=B)

    def run(self, B, tau, mode, source=None, **kw):
        return self.router(B, tau, mode).run(self.n, self.q, self.p, self.daily_q if source is None else source,
                                             self.n_days, **kw)

    def hourly_by_route(self, B, mode):
        """The period's hourly series through the existing path: route() per chunk, q0 carried, concatenated."""
        parts, q0 = [], None
        for first, last in period_chunks(self.n_days, B):
            runoff, q0, _, _ = route(self.graph, self.daily_q[first:last + 1], self.n, self.q, self.p, self.length,
                                     self.slope, self.x, q0=q0, gauges=self.gauges if mode == "gauge" else None,
                                     consts=CONSTS, steps=(last - first) * 24, qprime_hours=24)
            parts.append(runoff)
        return torch.cat(parts, dim=1)


@pytest.mark.parametrize("gkw", PARTITIONS, ids=["whole", "cut"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("B", CHUNK_DAYS)
def test_daily_matches_reference_and_oracle(cuda, B, tau, mode, gkw):
    s = Setup(cuda, gkw=gkw)
    daily = s.run(B, tau, mode).daily.cpu().numpy()
    ref = s.golden[f"daily_B{B}_tau{tau}_{mode}"]
    assert daily.shape == ref.shape
    e_ref, e_orc = maxrel(daily, ref), maxrel(daily, oracle_period(B, tau, mode)[0])
    print(f"B={B} tau={tau} {mode}: max-rel vs reference {e_ref:.3e}, vs oracle {e_orc:.3e}")
    assert e_ref <= 1e-4
    assert e_orc <= 1e-6


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("mode", MODES)
def test_daily_is_bitwise_the_pooled_hourly_path(cuda, mode, dtype):
    """route() per chunk with hourly output, concatenated, trimmed and pooled sequentially on the host in the
    series' own precision: the same bits, for a plan whose every chunk boundary splits a day."""
    s = Setup(cuda, dtype, PARTITIONS[1])
    for B, tau in ((3, 3), (2, 0)):
        hourly = s.hourly_by_route(B, mode)
        res = s.run(B, tau, mode, keep_hourly=mode == "gauge")
        assert res.daily.dtype == dtype
        want = pool_sequential(hourly.cpu().numpy(), tau)
        assert np.array_equal(res.daily.cpu().numpy(), want), (B, tau)
        if mode == "gauge":
            assert torch.equal(res.hourly, hourly)
        else:
            assert res.hourly is None
        # the state the period ends in is the last chunk's
        last = period_chunks(s.n_days, B)[-1]
        assert res.q_last.shape == (s.case.n,) and bool(torch.isfinite(res.q_last).all()), last


@pytest.mark.parametrize("first_hour", [13, 16, 23])
@pytest.mark.parametrize("h0", [0, 24, 40])
def test_straddle_bookkeeping_of_the_entry_point(cuda, h0, first_hour):
    """One launch of T = 72 hours placed at period hour h0: windows that start before, inside and after it.  A day is
    started from 0 only if the launch holds its first hour (else from what the buffer held), divided only if the
    launch holds its last hour, and not written at all if the launch holds none of its hours."""
    s = Setup(cuda, gkw=PARTITIONS[1])
    T, D = 72, 6
    qp = s.tt(np.repeat(s.store[:4], 24, axis=0)[:T])
    lib = _lib.load()
    stream = _lib.stream_ptr(cuda)
    for mode in MODES:
        gz = s.gauges if mode == "gauge" else None
        hourly, _, _, _, x_save, _ = mc_route(qp, s.n, s.q, s.p, s.length, s.slope, s.x, None, None,
                                              gz.offsets if gz else None, gz.index if gz else None, None, None, None,
                                              register_graph(s.graph), CONSTS.as_list(), _lib.DDR_FWD_SAVE_X, T, 1, [])
        hourly = hourly.cpu().numpy()
        R = hourly.shape[0]
        gzc = _lib.Gauges(R, gz.offsets.data_ptr(), gz.index.data_ptr(), None, None) if gz else None
        # (all-reach mode has two store variants: the LDS tile and the per-thread store kept for the A/B timing)
        runs = [(0.0, 0), (float("nan"), 0)] + ([] if gz else [(float("nan"), _lib.DDR_PERIOD_DIRECT_STORE)])
        for fill, flags in runs:
            buf = torch.full((R, D), fill, device=cuda, dtype=torch.float32)
            _lib.check(lib.ddr_period_daily_f32(s.graph.handle, x_save.data_ptr(), T, C.byref(gzc) if gzc else None,
                                                CONSTS.discharge_lb, flags, h0, first_hour, D, buf.data_ptr(), stream))
            got = buf.cpu().numpy()
            want = np.full((R, D), fill, np.float32)
            kinds = []
            for d in range(D):
                w0 = first_hour + 24 * d
                lo, hi = max(w0, h0), min(w0 + 24, h0 + T)
                if lo >= hi:
                    kinds.append("untouched")
                    continue
                acc = np.zeros(R, np.float32) if lo == w0 else want[:, d].copy()
                for h in range(lo, hi):
                    acc = acc + hourly[:, h - h0]
                want[:, d] = acc / np.float32(24) if hi == w0 + 24 else acc
                kinds.append("finished" if lo == w0 and hi == w0 + 24 else "partial")
            assert "finished" in kinds and "untouched" in kinds, kinds  # (h0 = 40, first_hour = 16: no partial day)
            assert np.array_equal(got, want, equal_nan=True), (mode, fill, kinds)
            if np.isnan(fill):
                for d, kind in enumerate(kinds):
                    if kind == "finished":
                        assert not np.isnan(got[:, d]).any()
                    if kind == "untouched":
                        assert np.isnan(got[:, d]).all()


def test_one_launch_meeting_more_days_than_a_tile(cuda):
    """T = 821 hours in one launch: 35 windows, more than the 32 days of one tile of the all-reach kernel, an odd
    T, 300 reaches (no multiple of the 64 positions of a tile); both store variants and the gauge rows against the
    sequential host pooling of the launch's hourly output."""
    s = Setup(cuda, gkw=PARTITIONS[1])
    T, D, first_hour = 821, 36, 16
    qp = s.tt(np.tile(np.repeat(s.store, 24, axis=0), (5, 1))[:T])
    lib = _lib.load()
    stream = _lib.stream_ptr(cuda)
    for mode in MODES:
        gz = s.gauges if mode == "gauge" else None
        hourly, _, _, _, x_save, _ = mc_route(qp, s.n, s.q, s.p, s.length, s.slope, s.x, None, None,
                                              gz.offsets if gz else None, gz.index if gz else None, None, None, None,
                                              register_graph(s.graph), CONSTS.as_list(), _lib.DDR_FWD_SAVE_X, T, 1, [])
        hourly = hourly.cpu().numpy()
        R = hourly.shape[0]
        want = np.full((R, D), np.nan, np.float32)
        for d in range(D):
            lo, hi = first_hour + 24 * d, min(first_hour + 24 * d + 24, T)
            if lo >= hi:
                continue
            acc = np.zeros(R, np.float32)
            for h in range(lo, hi):
                acc = acc + hourly[:, h]
            want[:, d] = acc / np.float32(24) if hi == lo + 24 else acc
        assert not np.isnan(want[:, :33]).any() and np.isnan(want[:, 34:]).all()  # day 33 is partial
        gzc = _lib.Gauges(R, gz.offsets.data_ptr(), gz.index.data_ptr(), None, None) if gz else None
        for flags in (0,) if gz else (0, _lib.DDR_PERIOD_DIRECT_STORE):
            buf = torch.full((R, D), float("nan"), device=cuda, dtype=torch.float32)
            _lib.check(lib.ddr_period_daily_f32(s.graph.handle, x_save.data_ptr(), T, C.byref(gzc) if gzc else None,
                                                CONSTS.discharge_lb, flags, 0, first_hour, D, buf.data_ptr(), stream))
            assert np.array_equal(buf.cpu().numpy(), want, equal_nan=True), (mode, flags)


def test_store_source_equals_its_daily_tensor(cuda):
    """A store that lacks a few divides (0.001 fill, valid mask) pulled chunk by chunk, against the whole period's
    window gathered once by the store's own daily()."""
    s = Setup(cuda)
    N, n_days, day0 = s.case.n, s.n_days, 2
    rng = np.random.default_rng(7)
    kept = np.sort(rng.permutation(N)[:N - 5])
    qr = rng.lognormal(0.0, 1.0, (kept.size, n_days + 4)).astype(np.float32)
    qr[:, day0:day0 + n_days] = s.store.T[kept]
    store = StreamflowStore(qr, kept + 1000, start="1980/01/01", device=cuda)
    rows = store.rows(np.arange(N) + 1000)
    assert int((rows < 0).sum()) == 5
    qd, valid = store.daily(rows, day0, n_days)
    for mode in MODES:
        a = s.run(3, 3, mode, source=(store, rows, day0))
        b = s.run(3, 3, mode, source=(qd, valid))
        assert torch.equal(a.daily, b.daily)
        assert torch.equal(a.q_last, b.q_last)
        assert not torch.equal(a.daily, s.run(3, 3, mode).daily)  # the filled divides matter


def test_metrics_from_observation_store(cuda):
    s = Setup(cuda)
    res = s.run(3, 3, "gauge")
    G, n_days, day0, warmup = len(s.outflow), s.n_days, 3, 1
    rng = np.random.default_rng(3)
    obs = rng.lognormal(np.log(5.0), 1.0, (G + 2, n_days + 6)).astype(np.float32)
    ids = np.arange(G + 2) + 7
    store = ObservationStore(obs, ids, device=cuda)
    pick = np.array([4, 0, 5, 2])
    rows = store.rows(ids[pick])
    m = res.metrics_from(store, rows, day0, warmup)
    target = obs[pick][:, day0 + 1:day0 + n_days - 1]  # obs[:, 1:-1] of the period's days
    want = Metrics(pred=res.daily[:, warmup:].contiguous(), target=torch.from_numpy(target[:, warmup:].copy()).to(cuda))
    assert m.nt == n_days - 2 - warmup
    for name in METRIC_NAMES:
        assert np.array_equal(getattr(m, name), getattr(want, name), equal_nan=True), name
    m2 = res.metrics(target, warmup)
    assert np.array_equal(m2.nse, want.nse, equal_nan=True)


def test_argument_errors_raise_before_any_launch(cuda):
    s = Setup(cuda, gkw=PARTITIONS[1])
    with pytest.raises(ValueError, match="keep_hourly"):
        s.run(3, 3, "all", keep_hourly=True)
    with pytest.raises(ValueError, match="rows"):
        s.run(3, 3, "all", source=s.daily_q[:-1])
    with pytest.raises(ValueError, match="rows"):
        s.run(3, 3, "gauge", source=s.tt(np.repeat(s.store, 24, axis=0)))  # n_days * 24 hourly rows: one day too many
    # a split graph: the receive memory is never touched, because nothing is launched
    lib = _lib.load()
    g = RiverGraph(s.case.n, s.case.rows, s.case.cols, **PARTITIONS[1])
    nb = C.c_int64()
    _lib.check(lib.ddr_xmem_bytes(0, 48, C.byref(nb)))
    mem = [torch.zeros(nb.value, device=cuda, dtype=torch.uint8) for _ in range(2)]
    block_rank = np.zeros(g.info.n_blocks, np.int32)
    peers = (C.c_void_p * 2)(mem[0].data_ptr(), mem[1].data_ptr())
    n_x = C.c_int64()
    _lib.check(lib.ddr_graph_set_split(g.handle, 0, 2, block_rank.ctypes.data, mem[0].data_ptr(), peers, 48,
                                       C.byref(n_x)))
    try:
        router = PeriodRouter(g, s.length, s.slope, s.x, consts=CONSTS, chunk_days=3)
        with pytest.raises(ValueError, match="split"):
            router.run(s.n, s.q, s.p, s.daily_q, s.n_days)
    finally:
        _lib.check(lib.ddr_graph_clear_split(g.handle))
    torch.cuda.synchronize()
    assert all(int(m.sum()) == 0 for m in mem)
