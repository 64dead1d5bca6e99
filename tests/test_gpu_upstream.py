"""The upstream index on the device (csrc/upstream.hip): every output against the host index and, directly, against
the independent expectations of upstream_cases.py (a brute-force sweep, the reference's own arrays in
tests/golden/collate.npz, the existing collate fed with sweep-built subsets)."""

import ctypes as C

import numpy as np
import pytest
import torch

import upstream_cases as U
from conftest import load_golden
from ddr_amd import _lib, synthetic
from ddr_amd.batching import collate_gauges, collate_gauges_device
from ddr_amd.graph import RiverGraph
from ddr_amd.upstream import UpstreamIndex

pytestmark = pytest.mark.gpu


def indices(down, cuda):
    rows, cols = U.coo_of(down)
    return UpstreamIndex(len(down), rows, cols), UpstreamIndex(len(down), rows, cols, device=cuda)


def test_small_cases_on_the_device(cuda):
    """Chains across the doubling-round boundaries, forests across the wave and block tails, no edges, gauges on
    outlets / headwaters / isolated reaches / one reach, nested, repeated, G = 0 and G = 300."""
    for name, down, gauges in U.small_cases():
        n = len(down)
        host, dev = indices(down, cuda)
        assert (dev.n, dev.n_outlets, dev.max_depth, dev.rounds) == (n, int((down < 0).sum()), U.depth_of(down),
                                                                     host.rounds), name
        np.testing.assert_array_equal(dev.down, down, err_msg=name)
        want = U.sweep_members(down, gauges)
        union = np.unique(np.concatenate(want)) if gauges else np.zeros(0, np.int64)
        np.testing.assert_array_equal(dev.closure(gauges), union, err_msg=name)
        label, slot_of = dev.label(gauges)
        hl, hs = host.label(gauges)
        np.testing.assert_array_equal(label.cpu().numpy(), hl, err_msg=name)
        np.testing.assert_array_equal(slot_of, hs, err_msg=name)
        off, idx = dev.members(gauges)
        U.check_members(off, idx, down, gauges)
        ho, hi = host.members(gauges)
        np.testing.assert_array_equal(off, ho, err_msg=name)
        np.testing.assert_array_equal(idx, hi, err_msg=name)
        db = dev.collate(gauges)
        assert db.active.is_cuda and db.active.dtype == torch.int32 and db.crow.dtype == torch.int64
        cb = db.to_host()
        U.check_batch_equal(cb, host.collate(gauges))
        U.check_batch_equal(cb, collate_gauges(n, U.expected_subsets(down, gauges)))
        for (r, c, g), (er, ec, eg) in zip(dev.subsets(gauges), U.expected_subsets(down, gauges)):
            assert g == eg
            np.testing.assert_array_equal(r, er)
            np.testing.assert_array_equal(c, ec)


def test_golden_batch_on_the_device(cuda):
    """The reference batch from the CONUS COO alone, against the reference's own arrays; its graph has the
    fingerprint of the graph built from the host union."""
    d = load_golden("collate")
    n = int(d["n_conus"])
    dev = UpstreamIndex(n, d["conus_rows"], d["conus_cols"], device=cuda)
    batch = U.golden_batch_gauges(d)
    db = dev.collate(batch)
    U.check_against_golden(db.to_host(), d)
    np.testing.assert_array_equal(dev.closure(batch), d["ref_divide_ids"] - 500000)
    off = d["sub_off"]
    keep = [(d["sub_rows"][off[g]:off[g + 1]], d["sub_cols"][off[g]:off[g + 1]], int(d["gage_idx"][g]))
            for g, b in enumerate(d["gage_ids"].tolist()) if b in d["batch"].tolist()]
    hn, hrows, hcols = collate_gauges(n, keep).coo()
    g = db.graph()
    assert g.device_built and g.fingerprint() == RiverGraph(hn, hrows, hcols).fingerprint()
    U.check_batch_equal(dev.subnetwork(batch).to_host(), db.to_host())


@pytest.fixture(scope="module")
def forest200k():
    net = synthetic.forest(synthetic.zipf_sizes(200_000, 400, 0.2), seed=5)
    gauges = np.random.default_rng(5).choice(np.flatnonzero(net.down >= 0), 64, replace=False).tolist()
    return net, gauges


def test_conus_scale_forest(cuda, forest200k):
    """64 nested interior gauges of a 200k-reach forest: the closure against one descending sweep, the union against
    the existing device collate fed with the host index's subsets, the member lists against the host index."""
    net, gauges = forest200k
    down = net.down
    host = UpstreamIndex(net.n, net.rows, net.cols)
    dev = UpstreamIndex(net.n, net.rows, net.cols, device=cuda)
    assert (dev.max_depth, dev.n_outlets, dev.rounds) == (host.max_depth, host.n_outlets, host.rounds)
    inside = np.zeros(net.n, bool)
    inside[gauges] = True
    for j in range(net.n - 1, -1, -1):
        if down[j] >= 0 and inside[down[j]]:
            inside[j] = True
    np.testing.assert_array_equal(dev.closure(gauges), np.flatnonzero(inside))
    subs = host.subsets(gauges)
    x = gauges[0]  # (one gauge's subset against its own sweep)
    np.testing.assert_array_equal(subs[0][1], U.expected_subsets(down, [x])[0][1])
    want = collate_gauges_device(net.n, subs, cuda).to_host()
    db = dev.collate(gauges)
    U.check_batch_equal(db.to_host(), want)
    np.testing.assert_array_equal(db.active.cpu().numpy(), np.flatnonzero(inside))
    off, idx = dev.members(gauges)
    ho, hi = host.members(gauges)
    np.testing.assert_array_equal(off, ho)
    np.testing.assert_array_equal(idx, hi)
    for g, (_, cols, reach) in enumerate(subs):
        assert off[g + 1] - off[g] == len(cols) + 1


def test_device_coo_input_equals_host_input(cuda, forest200k):
    net, gauges = forest200k
    a = UpstreamIndex(net.n, net.rows, net.cols, device=cuda)
    b = UpstreamIndex(net.n, torch.from_numpy(net.rows).to(cuda), torch.from_numpy(net.cols).to(cuda), device=cuda)
    assert (a.n, a.n_outlets, a.max_depth, a.rounds) == (b.n, b.n_outlets, b.max_depth, b.rounds)
    np.testing.assert_array_equal(a.down, b.down)
    np.testing.assert_array_equal(b.down, net.down)
    U.check_batch_equal(a.collate(gauges).to_host(), b.collate(gauges).to_host())
    # the device build refuses what the host build refuses; a duplicated edge passes; a network without edges
    t = lambda *v: torch.tensor(v, dtype=torch.int32, device=cuda)  # noqa: E731
    for rows, cols, code in (((1, 2), (0, 2), _lib.DDR_ERR_NOT_LOWER), ((1, 2), (0, 0), _lib.DDR_ERR_NOT_DENDRITIC),
                             ((1, 4), (0, 1), _lib.DDR_ERR_ARG)):
        with pytest.raises(_lib.DDRError) as e:
            UpstreamIndex(4, t(*rows), t(*cols), device=cuda)
        assert e.value.code == code
    np.testing.assert_array_equal(UpstreamIndex(4, t(1, 3, 1), t(0, 1, 0), device=cuda).down, [1, 3, -1, -1])
    empty = UpstreamIndex(3, t(), t(), device=cuda)
    assert (empty.max_depth, empty.n_outlets, empty.rounds) == (0, 3, 0)
    np.testing.assert_array_equal(empty.closure([2, 0]), [0, 2])


def test_device_queries_refuse_before_launching(cuda):
    """DDR_ERR_ARG with a message naming the fault; the outputs stay as they were."""
    lib = _lib.load()
    host, dev = indices(U.chain(5), cuda)
    h = dev._handle
    t = np.array([4, 1], np.int32)
    need = lib.ddr_upstream_scratch_bytes(h, 2, 0)
    assert need > 0 and lib.ddr_upstream_scratch_bytes(h, 2, 7) > need
    scratch = torch.empty(need // 8 + 1, dtype=torch.int64, device=cuda)
    label = torch.full((5,), 77, dtype=torch.int32, device=cuda)
    off = torch.full((3,), 77, dtype=torch.int64, device=cuda)
    total = C.c_int64(-5)
    s = _lib.stream_ptr(cuda)

    def refused(code, text):
        assert code == _lib.DDR_ERR_ARG
        assert text in lib.ddr_last_error().decode(), lib.ddr_last_error()

    refused(lib.ddr_upstream_label(h, 2, t.ctypes.data, label.data_ptr(), None, scratch.data_ptr(), need - 1, s),
            "scratch_bytes")
    refused(lib.ddr_upstream_label(h, 2, t.ctypes.data, label.data_ptr(), None, None, need, s), "null scratch")
    refused(lib.ddr_upstream_label(h, 2, t.ctypes.data, None, None, scratch.data_ptr(), need, s), "null label_out")
    refused(lib.ddr_upstream_label(h, -2, t.ctypes.data, label.data_ptr(), None, scratch.data_ptr(), need, s),
            "negative target count")
    refused(lib.ddr_upstream_label(h, 2, None, label.data_ptr(), None, scratch.data_ptr(), need, s), "null targets")
    bad = np.array([4, 5], np.int32)
    refused(lib.ddr_upstream_label(h, 2, bad.ctypes.data, label.data_ptr(), None, scratch.data_ptr(), need, s),
            "target 1 (reach 5) is outside [0, 5)")
    refused(lib.ddr_upstream_member_counts(h, 2, bad.ctypes.data, off.data_ptr(), C.byref(total), scratch.data_ptr(),
                                           need, s), "outside [0, 5)")
    refused(lib.ddr_upstream_member_counts(h, 2, t.ctypes.data, None, C.byref(total), scratch.data_ptr(), need, s),
            "null output")
    refused(lib.ddr_upstream_member_counts(h, 2, t.ctypes.data, off.data_ptr(), C.byref(total), scratch.data_ptr(), 8,
                                           s), "scratch_bytes")
    idx = torch.full((7,), 77, dtype=torch.int32, device=cuda)
    refused(lib.ddr_upstream_members(h, 2, t.ctypes.data, 7, idx.data_ptr(), scratch.data_ptr(), need, s),
            "scratch_bytes")  # (the sort's share is missing)
    refused(lib.ddr_upstream_members(h, 2, t.ctypes.data, -1, idx.data_ptr(), scratch.data_ptr(), need, s),
            "negative n_members")
    refused(lib.ddr_upstream_label(host._handle, 2, t.ctypes.data, label.data_ptr(), None, scratch.data_ptr(), need,
                                   s), "host-only")
    with pytest.raises(_lib.DDRError, match="outside"):
        dev.collate([9])
    torch.cuda.synchronize()
    assert total.value == -5
    assert label.eq(77).all() and off.eq(77).all() and idx.eq(77).all()
    # a wrong n_members is refused after the counts, before anything is emitted
    big = torch.empty(lib.ddr_upstream_scratch_bytes(h, 2, 9) // 8 + 1, dtype=torch.int64, device=cuda)
    idx9 = torch.full((9,), 77, dtype=torch.int32, device=cuda)
    refused(lib.ddr_upstream_members(h, 2, t.ctypes.data, 9, idx9.data_ptr(), big.data_ptr(), big.numel() * 8, s),
            "n_members 9 is not the 7")
    assert idx9.eq(77).all()
