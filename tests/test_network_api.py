"""The network build through its host twin (no GPU): the C ABI's refusals, every table of network_cases.py against
the plain-Python specification and networkx, and the ways into and out of :class:`ddr_amd.network.Network`."""

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import network_cases as N
from ddr_amd import _lib
from ddr_amd.network import Network, lookup, parse_ids

HEADER = Path(__file__).resolve().parents[1] / "include" / "ddr_mc.h"
ENTRY_POINTS = ("ddr_network_build", "ddr_network_build_host", "ddr_network_info", "ddr_network_get",
                "ddr_network_destroy", "ddr_network_lookup_i64", "ddr_network_lookup_i64_host")
CASES = N.small_cases()


def refused(code, text):
    assert code == _lib.DDR_ERR_ARG, (code, _lib.load().ddr_last_error())
    msg = _lib.load().ddr_last_error().decode()
    assert text in msg, msg


def test_header_and_binding_declare_the_entry_points():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    declared = set(re.findall(r"\b(ddr_[a-z0-9_]+)\s*\(", text))
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert name in declared and name in _lib.EXPORTED and hasattr(lib, name), name
    import ddr_amd

    assert ddr_amd.Network is Network


def test_refusals():
    """Null pointers, a negative n, an unknown flag, n too large: DDR_ERR_ARG naming the fault before anything is
    launched (there is no device here to launch on); a duplicated id by name."""
    lib = _lib.load()
    h = C.c_void_p()
    ids = np.array([5, 9, 7], np.int64)
    to = np.array([9, 0, 9], np.int64)
    p = lambda a: a.ctypes.data  # noqa: E731
    for build in (lambda *a: lib.ddr_network_build_host(*a, C.byref(h)),
                  lambda *a: lib.ddr_network_build(*a, 0, None, C.byref(h))):
        refused(build(3, None, p(to)), "null ids or to_ids")
        refused(build(3, p(ids), None), "null ids or to_ids")
        refused(build(-1, p(ids), p(to)), "negative row count")
        refused(build(1 << 30, p(ids), p(to)), "2^30 or more")
    refused(lib.ddr_network_build_host(3, p(ids), p(to), None), "null network pointer")
    refused(lib.ddr_network_build(3, p(ids), p(to), 0, None, None), "null network pointer")
    refused(lib.ddr_network_build(3, p(ids), p(to), 2, None, C.byref(h)), "unknown flag")
    dup = np.array([5, 9, 7, 9, 5], np.int64)
    refused(lib.ddr_network_build_host(5, p(dup), p(dup), C.byref(h)), "id 5 appears more than once")
    assert not h.value
    refused(lib.ddr_network_info(None, None), "null argument")
    refused(lib.ddr_network_get(None, None, None, None, None, None, None, None), "null network")
    pos = np.empty(3, np.int32)
    refused(lib.ddr_network_lookup_i64_host(-1, p(ids), 3, p(to), p(pos)), "negative count")
    refused(lib.ddr_network_lookup_i64_host(3, None, 3, p(to), p(pos)), "null ids")
    refused(lib.ddr_network_lookup_i64_host(3, p(ids), 3, p(to), None), "null queries or output")
    refused(lib.ddr_network_lookup_i64_host(5, p(dup), 3, p(to), p(pos)), "id 5 appears more than once")
    refused(lib.ddr_network_lookup_i64(3, p(ids), 3, p(to), p(pos), 4, None), "unknown flag")
    refused(lib.ddr_network_lookup_i64(1 << 30, p(ids), 3, p(to), p(pos), 0, None), "too large")
    with pytest.raises(_lib.DDRError, match="id 9 appears more than once"):
        Network.build([3, 9, 9], [0, 0, 0])
    with pytest.raises(ValueError, match="differ in length"):
        Network.build([3, 9], [0])
    with pytest.raises(TypeError, match="integers"):
        Network.build(np.array([1.5]), np.array([0]))
    assert lib.ddr_network_destroy(None) == 0


def test_lookup_and_parse_ids():
    ids = np.array([N.I64.min, -1, 0, N.I64.max, 7], np.int64)
    q = np.array([7, 8, N.I64.max, N.I64.min, N.I64.min + 1, 0, -1, -2], np.int64)
    got = lookup(ids, q)
    assert got.dtype == np.int32
    np.testing.assert_array_equal(got, [4, -1, 3, 0, -1, 2, 1, -1])
    assert len(lookup(ids, [])) == 0
    np.testing.assert_array_equal(lookup([], [3, 4]), [-1, -1])
    np.testing.assert_array_equal(parse_ids(["wb-12", "wb-7", None, ""], "wb-"), [12, 7, -1, -1])
    with pytest.raises(ValueError, match="does not start with"):
        parse_ids(["nex-3"], "wb-")


@pytest.mark.parametrize("name,ids,to", CASES, ids=[c[0] for c in CASES])
def test_small_cases(name, ids, to):
    want = N.specification(ids, to)
    cyc = N.networkx_dropped(ids, to)
    np.testing.assert_array_equal(want["dropped"], cyc)  # the specification and networkx agree on the cycles
    net = Network.build(ids, to)
    got = N.result_of(net)
    N.check_properties(got, ids, to, cyc)
    N.assert_same(got, want)
    assert net.n_rows == len(ids) and net.device is None and net.nnz == len(got["rows"])


def test_expected_shapes_of_the_cycle_cases():
    """What the tables were drawn to show, stated outright."""
    by = {c[0]: c for c in CASES}
    net = Network.build(*by["only-a-cycle"][1:])
    assert (net.n, net.nnz, net.n_basins, net.max_depth, len(net.dropped)) == (0, 0, 0, 0, 6)
    _, ids, to = by["cycle-tail5-branch"]
    net = Network.build(ids, to)
    assert len(net.dropped) == 4
    tail_last = int(np.flatnonzero(ids == 1500)[0])  # drained into the cycle: an outlet now
    k = int(np.flatnonzero(net.position == tail_last)[0])
    assert net.down[k] == -1
    kept_ids = set(net.ids.tolist())
    assert {1500, 1501, 1502, 1503, 1504, 1900, 1901} <= kept_ids  # the tail and both side reaches stay
    net = Network.build(*by["empty"][1:])
    assert (net.n, net.nnz, net.n_basins, net.max_depth, len(net.dropped)) == (0, 0, 0, 0, 0)
    net = Network.build(*by["reversed-chain4097"][1:])
    assert (net.n, net.nnz, net.n_basins, net.max_depth) == (4097, 4096, 1, 4096)
    np.testing.assert_array_equal(net.position, np.arange(4096, -1, -1))


def test_hundred_thousand_reaches():
    ids, to, want = N.big_case()
    N.assert_same(N.result_of(Network.build(ids, to)), want)
    assert len(want["dropped"]) == 0


def upstream_columns(ids, to):
    """The MERIT form of a table: per row the ids that drain into it."""
    down = N.down_rows(ids, to)
    k = int(np.bincount(down[down >= 0]).max())
    ups = np.zeros((len(ids), k), np.int64)
    fill = np.zeros(len(ids), np.int64)
    for i in np.flatnonzero(down >= 0):
        ups[down[i], fill[down[i]]] = ids[i]
        fill[down[i]] += 1
    return ups


def test_from_upstream_columns():
    ids, to, _ = N.shuffled_forest(3000, 4)
    want = N.result_of(Network.build(ids, to))
    ups = upstream_columns(ids, to)
    ups = np.concatenate([ups, np.full((len(ids), 1), -3), np.full((len(ids), 1), 77)], axis=1)  # empty; not a row
    N.assert_same(N.result_of(Network.from_upstream_columns(ids, ups)), want)
    # the same reach in one row twice is no fault; under two different rows it is, by name
    twice = np.concatenate([ups, ups[:, :1]], axis=1)
    N.assert_same(N.result_of(Network.from_upstream_columns(ids, twice)), want)
    r = int(np.flatnonzero(ups[:, 0] > 0)[0])
    other = (r + 1) % len(ids)
    bad = ups.copy()
    bad[other, -1] = ups[r, 0]
    with pytest.raises(ValueError, match=f"flowpath {ups[r, 0]} is listed as upstream of two different rows"):
        Network.from_upstream_columns(ids, bad)
    with pytest.raises(ValueError, match="must be"):
        Network.from_upstream_columns(ids, ups[:-1])


def test_from_nexus():
    ids, to, _ = N.shuffled_forest(3000, 5)
    want = N.result_of(Network.build(ids, to))
    nexus = 7_000_000_000 + np.random.default_rng(5).permutation(len(ids)).astype(np.int64)
    # later duplicates of a nexus id point elsewhere and must lose to the first; terminal nexuses name no flowpath
    nx_ids = np.concatenate([nexus, nexus[:40]])
    nx_to = np.concatenate([to, np.roll(ids, 1)[:40]])
    N.assert_same(N.result_of(Network.from_nexus(ids, nexus, nx_ids, nx_to)), want)
    names = [f"wb-{v}" for v in ids[:5]]
    np.testing.assert_array_equal(parse_ids(names, "wb-"), ids[:5])


def test_round_trips(tmp_path):
    import networkx as nx

    from ddr_amd.zarr_coo import coo_from_zarr

    ids, to, _ = N.shuffled_forest(3000, 6)
    small = ids - (1 << 33)                      # (the store's order array is int32)
    to_small = np.where(to > 5, to - (1 << 33), -1)
    net = Network.build(small, to_small)
    net.to_zarr(tmp_path / "conus", note="built here")
    n, rows, cols, _, order = coo_from_zarr(tmp_path / "conus")
    assert n == net.n
    np.testing.assert_array_equal(rows, net.rows)
    np.testing.assert_array_equal(cols, net.cols)
    np.testing.assert_array_equal(order, net.ids)
    with pytest.raises(ValueError, match="int32"):
        Network.build(ids, to).to_zarr(tmp_path / "wide")
    ix = net.upstream_index()
    np.testing.assert_array_equal(ix.down, net.down)
    assert (ix.n_outlets, ix.max_depth) == (net.n_basins, net.max_depth)
    # per gauge: everything upstream, as ids, against networkx on the table as it was given
    down = N.down_rows(small, to_small)
    g = nx.DiGraph()
    g.add_nodes_from(range(len(small)))
    g.add_edges_from((i, int(d)) for i, d in enumerate(down) if d >= 0)
    gauges = np.random.default_rng(6).choice(net.n, 10, replace=False)
    off, idx = ix.members(gauges)
    for k, gk in enumerate(gauges):
        row = int(net.position[gk])
        want = {int(small[r]) for r in nx.ancestors(g, row) | {row}}
        assert set(net.ids[idx[off[k]:off[k + 1]]].tolist()) == want
    # align: a table column in the network's order
    length = np.random.default_rng(7).uniform(1, 2, len(small))
    np.testing.assert_array_equal(net.align(length), length[net.position])
    block = np.arange(2 * len(small)).reshape(2, -1)
    np.testing.assert_array_equal(net.align(block, axis=1), block[:, net.position])
    graph = net.graph(host_only=True)
    assert (graph.n, graph.info.nnz, graph.info.n_basins) == (net.n, net.nnz, net.n_basins)
