"""The network build on the device (csrc/network.hip): every table of network_cases.py must come out bit-identical to
the host twin and to the plain-Python specification, through device tensors and through the C ABI's host-input form;
then one network built from a shuffled table is routed and compared with the oracle on the original order."""

import ctypes as C

import numpy as np
import pytest
import torch

import network_cases as N
from conftest import Case, maxrel, synthetic_case
from ddr_amd import _lib, synthetic
from ddr_amd.network import Network, lookup
from oracle import mc_oracle as O
from test_gpu_route import run_hip
from test_network_api import upstream_columns

pytestmark = pytest.mark.gpu

CASES = N.small_cases()


@pytest.mark.parametrize("name,ids,to", CASES, ids=[c[0] for c in CASES])
def test_small_cases(cuda, name, ids, to):
    want = N.specification(ids, to)
    net = Network.build(ids, to, device=cuda)
    assert net.device == cuda and all(getattr(net, k).device == cuda for k in N.FIELDS)
    got = N.result_of(net)
    N.check_properties(got, ids, to, want["dropped"])
    N.assert_same(got, want)
    N.assert_same(got, N.result_of(Network.build(ids, to)))


def test_hundred_thousand_reaches(cuda):
    ids, to, want = N.big_case()
    dev_ids, dev_to = torch.from_numpy(ids.copy()).to(cuda), torch.from_numpy(to.copy()).to(cuda)
    net = Network.build(dev_ids, dev_to)  # device tensors alone select the device build
    assert net.device == cuda
    N.assert_same(N.result_of(net), want)
    np.testing.assert_array_equal(dev_ids.cpu().numpy(), ids)  # the input is read, not written
    np.testing.assert_array_equal(dev_to.cpu().numpy(), to)


def test_c_abi_host_input_and_host_output(cuda):
    """flags = 0: host ids go up inside the call; ddr_network_get of a device build fills host arrays too."""
    lib = _lib.load()
    by = {c[0]: c for c in CASES}
    for name in ("forest3000-with-cycles", "reversed-chain65", "empty"):
        _, ids, to = by[name]
        ids, to = np.ascontiguousarray(ids), np.ascontiguousarray(to)
        want = N.specification(ids, to)
        h = C.c_void_p()
        info = _lib.NetworkCounts()
        with torch.cuda.device(cuda):
            st = _lib.stream_ptr(cuda)
            _lib.check(lib.ddr_network_build(len(ids), ids.ctypes.data if len(ids) else None,
                                             to.ctypes.data if len(ids) else None, 0, st, C.byref(h)))
            _lib.check(lib.ddr_network_info(h, C.byref(info)))
            assert (info.n, info.kept, info.nnz, info.n_dropped, info.n_basins, info.max_depth, info.device) == (
                len(ids), want["n"], len(want["rows"]), len(want["dropped"]), want["n_basins"], want["max_depth"],
                cuda.index)
            got = {k: np.empty(len(want[k]), want[k].dtype) for k in N.FIELDS}
            _lib.check(lib.ddr_network_get(h, *(got[k].ctypes.data for k in N.FIELDS), st))
            _lib.check(lib.ddr_network_destroy(h))
        for k in N.FIELDS:
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"{name} {k}")


def test_duplicate_and_lookup(cuda):
    with pytest.raises(_lib.DDRError, match="id 5 appears more than once"):
        Network.build([5, 9, 7, 9, 5], [0, 0, 0, 0, 0], device=cuda)
    ids = np.array([N.I64.min, -1, 0, N.I64.max, 7], np.int64)
    q = np.array([7, 8, N.I64.max, N.I64.min, N.I64.min + 1, 0, -1, -2], np.int64)
    got = lookup(ids, q, device=cuda)
    assert got.device == cuda and got.dtype == torch.int32
    np.testing.assert_array_equal(got.cpu().numpy(), [4, -1, 3, 0, -1, 2, 1, -1])
    assert lookup(ids, [], device=cuda).numel() == 0
    np.testing.assert_array_equal(lookup([], [3, 4], device=cuda).cpu().numpy(), [-1, -1])
    with pytest.raises(_lib.DDRError, match="id 9 appears more than once"):
        lookup([3, 9, 9], [1], device=cuda)
    # the host-input form of the C ABI
    lib = _lib.load()
    pos = np.empty(len(q), np.int32)
    with torch.cuda.device(cuda):
        _lib.check(lib.ddr_network_lookup_i64(len(ids), ids.ctypes.data, len(q), q.ctypes.data, pos.ctypes.data, 0,
                                              _lib.stream_ptr(cuda)))
    np.testing.assert_array_equal(pos, [4, -1, 3, 0, -1, 2, 1, -1])
    big_ids, big_to, _ = N.big_case()
    np.testing.assert_array_equal(lookup(big_ids, big_to, device=cuda).cpu().numpy(), lookup(big_ids, big_to))


def test_other_forms_on_the_device(cuda):
    ids, to, _ = N.shuffled_forest(3000, 4)
    want = N.specification(ids, to)
    ups = upstream_columns(ids, to)
    N.assert_same(N.result_of(Network.from_upstream_columns(ids, ups, device=cuda)), want)
    bad = np.concatenate([ups, np.zeros((len(ids), 1), np.int64)], axis=1)
    r = int(np.flatnonzero(ups[:, 0] > 0)[0])
    bad[(r + 1) % len(ids), -1] = ups[r, 0]
    with pytest.raises(ValueError, match=f"flowpath {ups[r, 0]} is listed as upstream of two different rows"):
        Network.from_upstream_columns(torch.from_numpy(ids).to(cuda), torch.from_numpy(bad).to(cuda))
    nexus = 7_000_000_000 + np.random.default_rng(5).permutation(len(ids)).astype(np.int64)
    nx_ids = np.concatenate([nexus, nexus[:40]])
    nx_to = np.concatenate([to, np.roll(ids, 1)[:40]])
    net = Network.from_nexus(ids, nexus, nx_ids, nx_to, device=cuda)
    N.assert_same(N.result_of(net), want)
    ix = net.upstream_index()
    np.testing.assert_array_equal(ix.down, want["down"])


def test_built_network_routes_like_the_original(cuda):
    """A forest in contract order, its rows shuffled into a table, built on the device and routed for T = 8: the
    discharge, mapped back by id, against the oracle on the original order at the forward parity test's tolerance
    (test_gpu_route.test_fp32_matches_oracle_recipe: max-rel <= 1e-6)."""
    net0 = synthetic.forest(synthetic.zipf_sizes(4000, 12, 0.4), seed=21, single_inflow=0.35)
    case = synthetic_case(net0, 8, 21)
    ids, to, row_of_reach = N.shuffled_forest(net0.n, 21, forest=net0.down)
    reach_of_row = np.argsort(row_of_reach)
    table = lambda a: np.take(a, reach_of_row, axis=-1)  # noqa: E731  (a per-reach array as a column of the table)
    nw = Network.build(ids, to, device=cuda)
    assert nw.n == net0.n and len(nw.dropped) == 0
    g = nw.graph()
    assert g.device_built
    built = Case(nw.n, nw.rows.cpu().numpy(), nw.cols.cpu().numpy(), nw.align(table(case.length)),
                 nw.align(table(case.slope)), nw.align(table(case.x)), nw.align(table(case.qprime), axis=1), case.W,
                 {k: nw.align(table(v)) for k, v in case.u.items()}, case.params)
    res = run_hip(built, cuda, grads=False, graph=g)
    # back by id: new reach k carries ids[k]; original reach j carries the id of its table row
    k_of_reach = lookup(nw.ids, ids[row_of_reach]).cpu().numpy()
    assert np.all(k_of_reach >= 0)
    r = res["reaches"]
    orig = O.Reaches(*(np.asarray(a)[k_of_reach] for a in (r.n, r.q, r.p, r.length, r.slope, r.x)))
    ref = O.route(case.network(), orig, case.qprime, case.bounds, dtype=np.float32)
    assert maxrel(res["runoff"][k_of_reach], ref["runoff"]) <= 1e-6
    assert maxrel(res["q_last"][k_of_reach], ref["q_last"]) <= 1e-6
