"""Shared pieces of tests/test_period_api.py and tests/test_gpu_period.py: the case of tests/golden/period.npz
(make_period_golden.py) and the reference's whole-period loop composed from the CPU oracle."""

from __future__ import annotations

from functools import lru_cache

import numpy as np

from conftest import PARAMS_DEFAULT, Case, load_golden
from ddr_amd import synthetic
from oracle import mc_oracle as O

CHUNK_DAYS, TAUS, MODES = (2, 3, 8), (0, 3), ("all", "gauge")


@lru_cache(maxsize=1)
def period_case():
    """(case, daily store (n_days, N), outflow_idx, fixture dict) of period.npz; the synthetic inputs are rebuilt
    from their seed and checked against the fixture's checksum."""
    d = load_golden("period")
    n, seed, n_days = int(d["n"]), int(d["seed"]), int(d["n_days"])
    net = synthetic.random_binary_tree(n, seed=seed)
    at = synthetic.reach_attributes(net.n, seed)
    u = synthetic.unit_parameters(net.n, seed)
    store = synthetic.lateral_inflow(net.n, n_days, seed)
    assert float(store.astype(np.float64).sum()) == float(d["store_sum"]), "synthetic q' changed"
    offs = d["outflow_offsets"]
    outflow = [d["outflow_flat"][offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]
    case = Case(net.n, net.rows, net.cols, at.length, at.slope, at.x, None, None, u, PARAMS_DEFAULT)
    return case, store, outflow, d


def reference_chunks(n_days: int, batch: int) -> list[tuple[int, int]]:
    """The reference's plan written as the loader builds it (sequential batches of day indices, the previous day
    prepended from the second batch on): (first, last) of every batch that routes at least one hour."""
    out = []
    for s in range(0, n_days, batch):
        idx = list(range(s, min(s + batch, n_days)))
        if 0 not in idx:
            idx.insert(0, idx[0] - 1)
        if len(idx) > 1:
            out.append((idx[0], idx[-1]))
    return out


@lru_cache(maxsize=None)
def oracle_hourly(batch: int):
    """All-reach hourly predictions (N, (n_days - 1) * 24) of the chunked loop through the oracle (fp32)."""
    case, store, _, _ = period_case()
    n_days = store.shape[0]
    net, r = case.network(), case.reaches()
    pred = np.zeros((case.n, (n_days - 1) * 24), np.float32)
    q0 = None
    for first, last in reference_chunks(n_days, batch):
        qp = np.repeat(store[first:last + 1], 24, axis=0)[:(last - first) * 24]
        res = O.route(net, r, qp, case.bounds, q0=q0)
        pred[:, first * 24:last * 24] = res["runoff"]
        q0 = res["q_last"]
    pred.setflags(write=False)
    return pred


@lru_cache(maxsize=None)
def oracle_period(batch: int, tau: int, mode: str):
    """(daily (R, n_days - 2), hourly (R, H)) of the oracle composition: trim [13 + tau : -11 + tau], pool to days."""
    _, _, outflow, _ = period_case()
    hourly = oracle_hourly(batch)
    if mode == "gauge":
        hourly = np.ascontiguousarray(O.gauge_reduce(np.ascontiguousarray(hourly.T), outflow).T)
    H = hourly.shape[1]
    sl = np.ascontiguousarray(hourly[:, 13 + tau:H - 11 + tau])
    daily = O.area_downsample(sl, sl.shape[1] // 24)
    daily.setflags(write=False)
    return daily, hourly


def pool_sequential(hourly: np.ndarray, tau: int) -> np.ndarray:
    """hourly (R, H) -> (R, H // 24 - 1): each day's 24 hours from hour 13 + tau summed in ascending order in the
    array's own precision, then divided by 24."""
    R, H = hourly.shape
    D = H // 24 - 1
    out = np.zeros((R, D), hourly.dtype)
    for d in range(D):
        acc = np.zeros(R, hourly.dtype)
        for h in range(13 + tau + 24 * d, 13 + tau + 24 * d + 24):
            acc = acc + hourly[:, h]
        out[:, d] = acc / hourly.dtype.type(24)
    return out
