"""Flowpath tables shared by test_network_api.py (host twin) and test_gpu_network.py (device build), with
expectations that never come from the code under test: :func:`specification` is a plain-Python rendering of the four
steps the C header states (a dict for the lookup, peeling of in-degree-0 reaches for the cycles -- what is never
peeled lies on one --, ``np.lexsort`` for the order), and ``networkx`` gives a second opinion on the cycles
(``simple_cycles``) and on the result (``is_directed_acyclic_graph``)."""

from __future__ import annotations

from functools import lru_cache

import numpy as np

import upstream_cases as U

I64 = np.iinfo(np.int64)
FIELDS = ("position", "ids", "down", "rows", "cols", "dropped")


def down_rows(ids, to_ids) -> np.ndarray:
    row_of = {int(v): i for i, v in enumerate(ids)}
    assert len(row_of) == len(ids), "the case's ids must be distinct"
    return np.array([row_of.get(int(t), -1) for t in to_ids], np.int64)


def specification(ids, to_ids) -> dict:
    ids = np.asarray(ids, np.int64)
    n = len(ids)
    down = down_rows(ids, to_ids)
    # cycles: peel reaches nothing drains into; a tree and every tail of a cycle peel away completely
    indeg = np.bincount(down[down >= 0], minlength=n)
    peeled = [i for i in range(n) if indeg[i] == 0]
    for i in peeled:  # (grows while it is read)
        d = down[i]
        if d >= 0:
            indeg[d] -= 1
            if indeg[d] == 0:
                peeled.append(int(d))
    kept = np.zeros(n, bool)
    kept[peeled] = True
    dropped = np.flatnonzero(~kept).astype(np.int32)
    down = np.where(kept & (down >= 0) & kept[np.maximum(down, 0)], down, -1)
    # a reach is peeled before the reach it drains into: backwards, dist and outlet are known when they are needed
    dist = np.zeros(n, np.int64)
    outlet = np.arange(n)
    for i in reversed(peeled):
        if down[i] >= 0:
            dist[i] = dist[down[i]] + 1
            outlet[i] = outlet[down[i]]
    is_outlet = kept & (down < 0)
    basin = (np.cumsum(is_outlet) - 1)[outlet]
    rows_kept = np.flatnonzero(kept)
    position = rows_kept[np.lexsort((rows_kept, -dist[rows_kept], basin[rows_kept]))]
    new_of = np.full(n, -1, np.int64)
    new_of[position] = np.arange(len(position))
    down_new = np.where(down[position] >= 0, new_of[np.maximum(down[position], 0)], -1)
    cols = np.flatnonzero(down_new >= 0)
    return dict(position=position.astype(np.int32), ids=ids[position], down=down_new.astype(np.int32),
                rows=down_new[cols].astype(np.int32), cols=cols.astype(np.int32), dropped=dropped, n=len(position),
                n_basins=int(is_outlet.sum()), max_depth=int(dist[kept].max()) if kept.any() else 0)


def networkx_dropped(ids, to_ids) -> np.ndarray:
    import networkx as nx

    down = down_rows(ids, to_ids)
    g = nx.DiGraph((i, int(d)) for i, d in enumerate(down) if d >= 0)
    return np.array(sorted({v for c in nx.simple_cycles(g) for v in c}), np.int32)


def result_of(net) -> dict:
    """A Network's arrays on the host."""
    host = lambda a: a if isinstance(a, np.ndarray) else a.cpu().numpy()  # noqa: E731
    out = {k: host(getattr(net, k)) for k in FIELDS}
    out.update(n=net.n, n_basins=net.n_basins, max_depth=net.max_depth)
    return out


def assert_same(got: dict, want: dict) -> None:
    for k in FIELDS:
        assert got[k].dtype == want[k].dtype, (k, got[k].dtype)
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    for k in ("n", "n_basins", "max_depth"):
        assert got[k] == want[k], (k, got[k], want[k])


def check_properties(got: dict, ids, to_ids, dropped_rows) -> None:
    """What must hold whatever the order."""
    import networkx as nx

    n = len(ids)
    down = down_rows(ids, to_ids)
    gone = np.zeros(n, bool)
    gone[dropped_rows] = True
    np.testing.assert_array_equal(got["dropped"], np.flatnonzero(gone))
    pos = got["position"].astype(np.int64)
    np.testing.assert_array_equal(np.sort(pos), np.flatnonzero(~gone))  # a permutation of the kept rows
    np.testing.assert_array_equal(got["ids"], np.asarray(ids, np.int64)[pos])
    rows, cols = got["rows"].astype(np.int64), got["cols"].astype(np.int64)
    assert np.all(rows > cols) and np.all(np.diff(cols) > 0)
    want_edges = {(i, int(d)) for i, d in enumerate(down) if d >= 0 and not gone[i] and not gone[d]}
    assert set(zip(pos[cols].tolist(), pos[rows].tolist())) == want_edges
    dn = got["down"].astype(np.int64)
    np.testing.assert_array_equal(dn[cols], rows)
    assert np.all(np.delete(dn, cols) == -1)
    assert got["n"] == len(pos) and got["n_basins"] == int((dn < 0).sum())
    assert got["max_depth"] == (U.depth_of(dn) if len(dn) else 0)
    g = nx.DiGraph(zip(cols.tolist(), rows.tolist()))
    assert nx.is_directed_acyclic_graph(g)


# ---- tables ---------------------------------------------------------------------------------------------------------
def reversed_chain(length: int):
    """Row r holds the reach r hops above the outlet: the order the contract forbids, exactly reversed."""
    ids = 10 + np.arange(length, dtype=np.int64)
    to = ids - 1
    to[0] = 0
    return ids, to


def star(inflows: int):
    """``inflows`` reaches into one hub that sits in the middle row."""
    ids = 100 + np.arange(inflows + 1, dtype=np.int64)
    hub = inflows // 2
    to = np.full(inflows + 1, ids[hub])
    to[hub] = -5
    return ids, to


def shuffled_forest(n: int, seed: int, forest=None):
    """A dendritic forest in contract order, its rows shuffled: ids above 32 bits, non-monotone and non-dense; the
    outlets' to_ids vary between 0, -1 and a foreign id.  Returns (ids, to_ids, row_of_reach)."""
    down = U.random_forest(n, seed) if forest is None else np.asarray(forest, np.int64)
    rng = np.random.default_rng(seed + 50_000)
    reach_id = rng.permutation(n).astype(np.int64) * 7919 + (1 << 33)
    outlet_to = np.array([0, -1, 5], np.int64)[rng.integers(0, 3, n)]
    reach_to = np.where(down >= 0, reach_id[np.maximum(down, 0)], outlet_to)
    reach_of_row = rng.permutation(n)
    row_of_reach = np.empty(n, np.int64)
    row_of_reach[reach_of_row] = np.arange(n)
    return reach_id[reach_of_row], reach_to[reach_of_row], row_of_reach


def extremes():
    ids = np.array([I64.min, -1, 0, I64.max, 7], np.int64)
    to = np.array([-1, 0, I64.max, 12345, I64.min], np.int64)  # 7 -> MIN -> -1 -> 0 -> MAX -> (outlet)
    return ids, to


def cycle_table(length: int, tail: int = 0, branch: bool = False, base: int = 1000):
    """A cycle of ``length`` reaches (1: a self-loop); a tail of ``tail`` reaches draining into it and, with
    ``branch``, a reach draining into the tail's middle and one straight into the cycle.  Rows: tail head first."""
    cyc = base + np.arange(length, dtype=np.int64)
    ids = list(cyc)
    to = list(np.roll(cyc, -1))
    prev = int(cyc[length // 2])
    for k in range(tail):  # built from the cycle upwards
        ids.append(base + 500 + k)
        to.append(prev)
        prev = base + 500 + k
    if branch:
        ids += [base + 900, base + 901]
        to += [base + 500 + tail // 2 if tail else int(cyc[0]), int(cyc[0])]
    return np.array(ids[::-1], np.int64), np.array(to[::-1], np.int64)


def joined(*tables):
    return np.concatenate([t[0] for t in tables]), np.concatenate([t[1] for t in tables])


def small_cases() -> list:
    """[(name, ids, to_ids)]"""
    e = np.zeros(0, np.int64)
    cases = [("empty", e, e), ("one", np.array([42], np.int64), np.array([0], np.int64)),
             ("two-isolated", np.array([9, 3], np.int64), np.array([0, -1], np.int64))]
    # a power of two and one past it against the round count; more than one workgroup
    cases += [(f"reversed-chain{k}", *reversed_chain(k)) for k in (2, 3, 64, 65, 1025, 4097)]
    cases += [(f"star{k}", *star(k)) for k in (3, 4, 300)]
    cases += [(f"forest3000-seed{s}", *shuffled_forest(3000, s)[:2]) for s in (1, 2, 3)]
    cases.append(("int64-extremes", *extremes()))
    quiet = reversed_chain(5)
    cases.append(("self-loop", *joined(quiet, cycle_table(1, tail=2))))
    cases.append(("two-cycle", *joined(cycle_table(2, tail=1), quiet)))
    cases += [(f"cycle{k}", *joined(quiet, cycle_table(k, tail=3))) for k in (3, 5, 7)]
    cases.append(("cycle-tail5-branch", *joined(cycle_table(4, tail=5, branch=True), quiet)))
    cases.append(("two-cycles", *joined(cycle_table(3, tail=2), quiet, cycle_table(5, tail=1, branch=True, base=5000))))
    cases.append(("only-a-cycle", *cycle_table(6)))
    f = shuffled_forest(3000, 7)
    ids, to = f[0].copy(), f[1].copy()
    d = down_rows(ids, to)
    out = [i for i in np.flatnonzero(d < 0) if np.any(d == i)]  # outlets something drains into
    to[out[0]] = ids[out[0]]   # an outlet turned self-loop: its inflows become outlets
    inflow = np.flatnonzero(d == out[1])[0]
    above = np.flatnonzero(d == inflow)
    to[out[1]] = ids[above[0] if len(above) else inflow]  # a 3- (or 2-) cycle through an outlet and what drains into it
    cases.append(("forest3000-with-cycles", ids, to))
    return cases


@lru_cache(maxsize=None)
def big_case():
    """(ids, to_ids, specification): one 100 000-reach shuffled forest, for the multi-block sort and scan paths."""
    ids, to, _ = shuffled_forest(100_000, 11)
    for a in (ids, to):
        a.setflags(write=False)
    return ids, to, specification(ids, to)
