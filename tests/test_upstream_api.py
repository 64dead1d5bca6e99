"""The upstream index through its host twin (no GPU): the C ABI's refusals, the golden batch of
tests/golden/collate.npz (the reference's own ``construct_network_matrix`` / ``_collate_gages`` results and the
engine-style subsets), and closures / member lists against ``networkx.ancestors`` and a brute-force sweep."""

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import upstream_cases as U
from conftest import load_golden
from ddr_amd import _lib
from ddr_amd.batching import collate_gauges
from ddr_amd.upstream import UpstreamIndex

HEADER = Path(__file__).resolve().parents[1] / "include" / "ddr_mc.h"
ENTRY_POINTS = ("ddr_upstream_index_create", "ddr_upstream_index_destroy", "ddr_upstream_index_info",
                "ddr_upstream_index_down", "ddr_upstream_scratch_bytes", "ddr_upstream_label", "ddr_upstream_collate",
                "ddr_upstream_member_counts", "ddr_upstream_members", "ddr_upstream_label_host",
                "ddr_upstream_collate_host", "ddr_upstream_member_counts_host", "ddr_upstream_members_host")
CASES = U.small_cases()


def host_index(down) -> UpstreamIndex:
    rows, cols = U.coo_of(down)
    return UpstreamIndex(len(down), rows, cols)


def refused(code, want, text):
    assert code == want, (code, _lib.load().ddr_last_error())
    msg = _lib.load().ddr_last_error().decode()
    assert text in msg, msg


def test_header_and_binding_declare_the_entry_points():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    declared = set(re.findall(r"\b(ddr_[a-z0-9_]+)\s*\(", text))
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert name in declared and name in _lib.EXPORTED and hasattr(lib, name), name


def test_index_create_refusals():
    lib = _lib.load()
    h = C.c_void_p()
    i32 = lambda *a: np.array(a, np.int32)  # noqa: E731
    HOST = _lib.DDR_UPSTREAM_HOST_ONLY

    def create(n, rows, cols, flags=HOST, e=None, out=h):
        return lib.ddr_upstream_index_create(n, len(rows) if e is None else e, rows.ctypes.data if len(rows) else None,
                                             cols.ctypes.data if len(cols) else None, flags, None,
                                             C.byref(out) if out is not None else None)

    refused(create(0, i32(), i32()), _lib.DDR_ERR_ARG, "at least one reach")
    refused(create(4, i32(), i32(), e=-1), _lib.DDR_ERR_ARG, "negative edge count")
    refused(create(4, i32(), i32(), e=2), _lib.DDR_ERR_ARG, "null COO")
    refused(create(4, i32(1), i32(0), out=None), _lib.DDR_ERR_ARG, "null index pointer")
    refused(create(4, i32(1), i32(0), flags=64), _lib.DDR_ERR_ARG, "unknown flag")
    refused(create(4, i32(1), i32(0), flags=HOST | _lib.DDR_UPSTREAM_DEVICE_COO), _lib.DDR_ERR_ARG, "host-only")
    refused(create(4, i32(4), i32(0)), _lib.DDR_ERR_ARG, "out of range")
    refused(create(4, i32(1, 2), i32(0, 2)), _lib.DDR_ERR_NOT_LOWER, "(2,2) is not strictly lower triangular")
    refused(create(4, i32(1, 1), i32(0, 3)), _lib.DDR_ERR_NOT_LOWER, "(1,3) is not strictly lower triangular")
    refused(create(4, i32(1, 2), i32(0, 0)), _lib.DDR_ERR_NOT_DENDRITIC, "reach 0 drains into 1 and 2")
    assert not h.value
    # the same edge twice is accepted, as the batch union accepts it
    ix = UpstreamIndex(4, i32(1, 3, 1), i32(0, 1, 0))
    np.testing.assert_array_equal(ix.down, [1, 3, -1, -1])
    assert (ix.n, ix.n_outlets, ix.max_depth, ix.rounds) == (4, 2, 2, 2)
    with pytest.raises(_lib.DDRError) as e:
        UpstreamIndex(4, i32(1, 2), i32(0, 0))
    assert e.value.code == _lib.DDR_ERR_NOT_DENDRITIC


def test_query_refusals():
    """Null pointers, negative counts, a target outside [0, n), a host-only index given to a device query: each
    DDR_ERR_ARG with a message naming the fault; nothing is launched (there is no device here to launch on)."""
    lib = _lib.load()
    ix = host_index(U.chain(5))
    h = ix._handle
    t = np.array([4, 1], np.int32)
    label = np.empty(5, np.int32)
    slot = np.empty(2, np.int32)
    off = np.empty(3, np.int64)
    E = _lib.DDR_ERR_ARG
    refused(lib.ddr_upstream_label_host(None, 2, t.ctypes.data, label.ctypes.data, slot.ctypes.data), E, "null index")
    refused(lib.ddr_upstream_label_host(h, -1, t.ctypes.data, label.ctypes.data, slot.ctypes.data), E,
            "negative target count")
    refused(lib.ddr_upstream_label_host(h, 2, None, label.ctypes.data, slot.ctypes.data), E, "null targets")
    refused(lib.ddr_upstream_label_host(h, 2, t.ctypes.data, None, slot.ctypes.data), E, "null label_out")
    for bad in (5, -1):
        tb = np.array([4, bad], np.int32)
        refused(lib.ddr_upstream_label_host(h, 2, tb.ctypes.data, label.ctypes.data, slot.ctypes.data), E,
                f"target 1 (reach {bad}) is outside [0, 5)")
        refused(lib.ddr_upstream_member_counts_host(h, 2, tb.ctypes.data, off.ctypes.data), E, "outside [0, 5)")
    refused(lib.ddr_upstream_member_counts_host(h, 2, t.ctypes.data, None), E, "null off")
    refused(lib.ddr_upstream_member_counts_host(h, -3, t.ctypes.data, off.ctypes.data), E, "negative target count")
    assert lib.ddr_upstream_member_counts_host(h, 2, t.ctypes.data, off.ctypes.data) == 0
    np.testing.assert_array_equal(off, [0, 5, 7])
    refused(lib.ddr_upstream_members_host(h, 2, t.ctypes.data, off.ctypes.data, None), E, "null argument")
    wrong = np.array([0, 4, 7], np.int64)
    idx = np.empty(7, np.int32)
    refused(lib.ddr_upstream_members_host(h, 2, t.ctypes.data, wrong.ctypes.data, idx.ctypes.data), E,
            "off is not what ddr_upstream_member_counts gives")
    na, nnz = C.c_int64(), C.c_int64()
    act, col, oi, gc = (np.empty(8, np.int32) for _ in range(4))
    crow = np.empty(6, np.int64)
    collate = lambda G, tp, acap=5, ecap=5, a=act.ctypes.data: lib.ddr_upstream_collate_host(  # noqa: E731
        h, G, tp, a, acap, C.byref(na), crow.ctypes.data, col.ctypes.data, ecap, C.byref(nnz), off.ctypes.data,
        oi.ctypes.data, 8, gc.ctypes.data)
    refused(collate(-1, t.ctypes.data), E, "negative target count")
    refused(collate(2, None), E, "null targets")
    refused(collate(2, t.ctypes.data, a=None), E, "null output")
    refused(collate(2, t.ctypes.data, acap=-1), E, "negative capacity")
    refused(collate(2, t.ctypes.data, acap=4), E, "exceed active_cap")
    refused(collate(2, t.ctypes.data, ecap=3), E, "exceed edge_cap")
    assert collate(2, t.ctypes.data) == 0 and (na.value, nnz.value) == (5, 4)
    # a host-only index serves no device query, and has no device scratch
    assert lib.ddr_upstream_scratch_bytes(h, 2, 0) == 0
    assert lib.ddr_upstream_scratch_bytes(None, 2, 0) == -1 and lib.ddr_upstream_scratch_bytes(h, -1, 0) == -1
    dummy = np.empty(64, np.int64)
    refused(lib.ddr_upstream_label(h, 2, t.ctypes.data, label.ctypes.data, slot.ctypes.data, dummy.ctypes.data, 512,
                                   None), E, "host-only")
    refused(lib.ddr_upstream_member_counts(h, 2, t.ctypes.data, off.ctypes.data, C.byref(na), dummy.ctypes.data, 512,
                                           None), E, "host-only")
    refused(lib.ddr_upstream_members(h, 2, t.ctypes.data, 7, idx.ctypes.data, dummy.ctypes.data, 512, None), E,
            "host-only")
    refused(lib.ddr_upstream_collate(h, 2, t.ctypes.data, act.ctypes.data, 5, C.byref(na), act.ctypes.data,
                                     act.ctypes.data, 5, C.byref(nnz), crow.ctypes.data, col.ctypes.data,
                                     off.ctypes.data, oi.ctypes.data, 8, gc.ctypes.data, dummy.ctypes.data, 512, None),
            E, "host-only")
    refused(lib.ddr_upstream_label(None, 2, t.ctypes.data, label.ctypes.data, slot.ctypes.data, dummy.ctypes.data, 512,
                                   None), E, "null index")
    refused(lib.ddr_upstream_index_info(h, None), E, "null argument")
    with pytest.raises(_lib.DDRError, match="outside"):
        ix.collate([7])
    with pytest.raises(ValueError, match="int32"):
        ix.members([1 << 32])


def test_golden_subsets_and_collate():
    """From the golden's CONUS COO alone: the engine-style subsets of every gauge, and the reference's own collate
    results for the batch."""
    d = load_golden("collate")
    ix = UpstreamIndex(int(d["n_conus"]), d["conus_rows"], d["conus_cols"])
    gauges = [int(g) for g in d["gage_idx"]]
    subs = ix.subsets(gauges)
    off = d["sub_off"]
    assert len(subs) == len(gauges)
    for g, (rows, cols, gi) in enumerate(subs):
        assert gi == gauges[g] and rows.dtype == np.int32 and cols.dtype == np.int32
        want = sorted(zip(d["sub_rows"][off[g]:off[g + 1]].tolist(), d["sub_cols"][off[g]:off[g + 1]].tolist()))
        assert sorted(zip(rows.tolist(), cols.tolist())) == want  # (the golden permutes its pairs)
    batch = U.golden_batch_gauges(d)
    cb = ix.collate(batch)
    U.check_against_golden(cb, d)
    assert cb.n_conus == int(d["n_conus"])
    # target-catchments mode: the same union
    U.check_batch_equal(ix.subnetwork(batch), cb)
    np.testing.assert_array_equal(ix.closure(batch), d["ref_divide_ids"] - 500000)


@pytest.mark.parametrize("name,down,gauges", CASES, ids=[c[0] for c in CASES])
def test_small_cases(name, down, gauges):
    ix = host_index(down)
    n = len(down)
    assert ix.n == n and ix.n_outlets == int((down < 0).sum())
    depth = U.depth_of(down)
    assert ix.max_depth == depth
    # 2^rounds hops carry the deepest reach past its outlet: rounds = ceil(log2(max_depth)) + 1
    assert ix.rounds == (0 if depth == 0 else int(np.ceil(np.log2(depth))) + 1)
    np.testing.assert_array_equal(ix.down, down)
    want = U.sweep_members(down, gauges)
    if n <= 300:
        for a, b in zip(U.networkx_members(down, gauges), want):
            np.testing.assert_array_equal(a, b)
    union = np.unique(np.concatenate(want)) if gauges else np.zeros(0, np.int64)
    np.testing.assert_array_equal(ix.closure(gauges), union)
    off, idx = ix.members(gauges)
    U.check_members(off, idx, down, gauges)
    # label: the nearest target at or downstream, the smallest slot of a shared reach
    label, slot_of = ix.label(gauges)
    first = {}
    for g, x in enumerate(gauges):
        first.setdefault(x, g)
    np.testing.assert_array_equal(slot_of, [first[x] for x in gauges])
    for i in range(n):
        j = i
        while j >= 0 and j not in first:
            j = int(down[j])
        assert label[i] == (first[j] if j >= 0 else -1), i
    # subsets in the engine's format, and the union the existing collate forms from them
    exp = U.expected_subsets(down, gauges)
    for (r, c, g), (er, ec, eg) in zip(ix.subsets(gauges), exp):
        assert g == eg
        np.testing.assert_array_equal(c, ec)
        np.testing.assert_array_equal(r, er)
    U.check_batch_equal(ix.collate(gauges), collate_gauges(n, exp))


def test_summed_q_prime_accepts_the_member_lists():
    from ddr_amd.validation import SummedQPrime

    down = U.random_forest(257, seed=77)
    gauges = [200, 13, 256, 13, 90]
    off, idx = host_index(down).members(gauges)
    s = SummedQPrime(off, idx)
    assert s.n_gauges == 5 and s.max_index == int(idx.max())


def test_subsets_write_a_gages_adjacency_store(tmp_path):
    """``subsets`` feeds ``gauge_subsets_to_zarr``; ``from_zarr`` reads a conus_adjacency store."""
    from ddr_amd.batching import collate_batch
    from ddr_amd.zarr_coo import coo_to_zarr, gauge_subsets_to_zarr, read_zarr

    d = load_golden("collate")
    n = int(d["n_conus"])
    coo_to_zarr(tmp_path / "conus", n, d["conus_rows"], d["conus_cols"])
    ix = UpstreamIndex.from_zarr(tmp_path / "conus")
    ids = d["gage_ids"].tolist()
    subs = ix.subsets([int(g) for g in d["gage_idx"]])
    gauge_subsets_to_zarr(tmp_path / "gages", n, {i: (r, c, g, None) for i, (r, c, g) in zip(ids, subs)})
    cb = collate_batch(d["batch"], read_zarr(tmp_path / "gages"))
    U.check_against_golden(cb, d)
