"""Small networks and gauge lists shared by test_upstream_api.py (host index) and test_gpu_upstream.py (device
index), with expectations that never come from the code under test: a brute-force descending sweep per gauge
(upstream reaches are numbered first, so ``inside[j] = inside[down[j]]`` visited downwards is exact) and
``networkx.ancestors``."""

from __future__ import annotations

import numpy as np


def coo_of(down):
    down = np.asarray(down, np.int64)
    cols = np.flatnonzero(down >= 0).astype(np.int32)
    return down[cols].astype(np.int32), cols


def chain(length: int) -> np.ndarray:
    down = np.arange(1, length + 1, dtype=np.int64)
    down[-1] = -1
    return down


def random_forest(n: int, seed: int, reach: int = 9, outlet_p: float = 0.08) -> np.ndarray:
    """A random dendritic forest: reach i drains into one of the next ``reach`` reaches, or nowhere."""
    rng = np.random.default_rng(seed)
    down = np.full(n, -1, np.int64)
    for i in range(n - 1):
        if rng.random() >= outlet_p:
            down[i] = rng.integers(i + 1, min(n, i + 1 + reach))
    return down


def sweep_members(down, gauges) -> list:
    """Per gauge: ascending ids of its reach and everything upstream of it."""
    down = np.asarray(down, np.int64)
    out = []
    for x in gauges:
        inside = np.zeros(len(down), bool)
        inside[x] = True
        for j in range(int(x) - 1, -1, -1):
            if down[j] >= 0 and inside[down[j]]:
                inside[j] = True
        out.append(np.flatnonzero(inside).astype(np.int64))
    return out


def networkx_members(down, gauges) -> list:
    import networkx as nx

    g = nx.DiGraph()
    g.add_nodes_from(range(len(down)))
    g.add_edges_from((i, int(d)) for i, d in enumerate(down) if d >= 0)
    return [np.array(sorted(nx.ancestors(g, int(x)) | {int(x)}), np.int64) for x in gauges]


def depth_of(down) -> int:
    down = np.asarray(down, np.int64)
    depth = np.zeros(len(down), np.int64)
    for i in range(len(down) - 1, -1, -1):
        if down[i] >= 0:
            depth[i] = depth[down[i]] + 1
    return int(depth.max())


def expected_subsets(down, gauges) -> list:
    """The engine's per-gauge COO from the sweep: every edge inside the gauge's closure."""
    down = np.asarray(down, np.int64)
    subs = []
    for x, m in zip(gauges, sweep_members(down, gauges)):
        cols = m[m != x]
        subs.append((down[cols].astype(np.int32), cols.astype(np.int32), int(x)))
    return subs


def small_cases() -> list:
    """[(name, down, gauges)]"""
    cases = []
    # doubling-round boundaries: chains with the target at the outlet, the head and the middle
    for length in (1, 2, 3, 4, 5, 63, 64, 65, 1025):
        d = chain(length)
        for where, t in (("outlet", length - 1), ("head", 0), ("middle", length // 2)):
            cases.append((f"chain{length}-{where}", d, [t]))
    # wave and block tails
    for n in (1, 63, 64, 65, 255, 256, 257):
        d = random_forest(n, seed=n)
        rng = np.random.default_rng(1000 + n)
        cases.append((f"forest{n}", d, rng.choice(n, size=min(n, 7), replace=False).tolist()))
    cases.append(("no-edges", np.full(7, -1, np.int64), [3, 0, 6]))
    #  0 -> 2 <- 1, 2 -> 4 <- 3 (4 an outlet), 5 isolated, 6 -> 7 (a second basin)
    d = np.array([2, 2, 4, 4, -1, -1, 7, -1], np.int64)
    cases.append(("outlet-gauge", d, [4]))
    cases.append(("headwater-gauge", d, [1]))
    cases.append(("isolated-gauge", d, [5]))
    cases.append(("outlet-headwater-isolated", d, [4, 1, 5, 7]))
    cases.append(("two-on-one-reach", d, [2, 2]))
    cases.append(("many-on-confluences", d, [2] * 20 + [4] * 20 + [7, 5]))  # (more outflow entries than n + G)
    cases.append(("nested-five", chain(40), [39, 30, 17, 5, 0]))
    f = random_forest(257, seed=77)
    cases.append(("unsorted-repeated", f, [200, 13, 256, 13, 90, 200, 4]))
    cases.append(("no-gauges", f, []))
    cases.append(("gauges-300", f, np.random.default_rng(300).integers(0, 257, 300).tolist()))
    return cases


def check_members(off, idx, down, gauges) -> None:
    """(off, idx) against the sweep: ascending lists that contain the gauge reach."""
    want = sweep_members(down, gauges)
    off = np.asarray(off)
    idx = np.asarray(idx)
    assert off.dtype == np.int64 and idx.dtype == np.int32
    assert off.shape == (len(gauges) + 1,) and off[0] == 0 and off[-1] == len(idx)
    for g, x in enumerate(gauges):
        got = idx[off[g]:off[g + 1]]
        np.testing.assert_array_equal(got, want[g])
        assert x in got and np.all(np.diff(got) > 0)


def check_batch_equal(a, b) -> None:
    """Two CollatedBatch objects hold the same union."""
    np.testing.assert_array_equal(a.active, b.active)
    np.testing.assert_array_equal(a.crow, b.crow)
    np.testing.assert_array_equal(a.col, b.col)
    assert a.gage_compressed_indices == b.gage_compressed_indices
    assert a.gage_idx == b.gage_idx
    assert len(a.outflow_idx) == len(b.outflow_idx)
    for x, y in zip(a.outflow_idx, b.outflow_idx):
        np.testing.assert_array_equal(x, y)


def check_against_golden(cb, d) -> None:
    """As tests/test_batching.py checks collate_gauges against the reference's own arrays."""
    np.testing.assert_array_equal(cb.active, d["ref_divide_ids"] - 500000)
    np.testing.assert_array_equal(cb.crow, d["ref_crow"])
    np.testing.assert_array_equal(cb.col, d["ref_col"])
    assert cb.gage_idx == d["ref_gage_idx"].tolist()
    assert cb.gage_compressed_indices == np.searchsorted(cb.active, d["ref_gage_idx"]).tolist()
    roff = d["ref_outflow_off"]
    assert len(cb.outflow_idx) == len(roff) - 1
    for g, o in enumerate(cb.outflow_idx):
        np.testing.assert_array_equal(o, np.sort(d["ref_outflow_flat"][roff[g]:roff[g + 1]]))


def golden_batch_gauges(d) -> list:
    batch = d["batch"].tolist()
    return [int(d["gage_idx"][i]) for i, b in enumerate(d["gage_ids"].tolist()) if b in batch]
