"""``ddr_amd.validation.linear_baseline``: the union of the gauges' subnetworks routed once gives, bit for bit, what
each gauge's own subnetwork routed alone gives (a reach's discharge depends only on what lies upstream of it);
headwater gauges are NaN rows exactly when skipped; the daily series is the hourly one pooled with PyTorch; the
hourly rows are the host model's."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import linear_cases as LC
import time_axis_cases as TA
from ddr_amd.io.stores import StreamflowStore
from ddr_amd.upstream import UpstreamIndex
from ddr_amd.validation import linear_baseline, metrics_device

pytestmark = pytest.mark.gpu

T, TAU = 96, 3


@pytest.fixture(scope="module")
def setup(cuda):
    net = TA.network("S")
    down = np.asarray(net.down)
    indeg = np.bincount(down[down >= 0], minlength=net.n)
    # 8 nested gauges: the outlet, a path of five reaches below one headwater, that headwater and another one
    heads = np.flatnonzero(indeg == 0)
    path = [int(heads[0])]
    while down[path[-1]] >= 0:
        path.append(int(down[path[-1]]))
    inner = [p for p in path[1:-1] if indeg[p] > 0][:5]
    gauges = np.array([path[-1]] + inner + [int(heads[0]), int(heads[-1])], np.int64)
    assert len(gauges) == 8 and len(set(gauges.tolist())) == 8
    index = UpstreamIndex(net.n, net.rows, net.cols, device=cuda)
    ids = np.arange(net.n, dtype=np.int64) * 7 + 3
    qr = np.random.default_rng(31).uniform(0.0, 2.0, (net.n - 4, T + 30)).astype(np.float32)
    store = StreamflowStore(qr, ids[:-4][::-1].copy(), is_hourly=True, device=cuda)  # four divides missing: the fill
    rows = store.align(ids)
    return net, indeg, gauges, index, store, rows


def test_union_equals_each_gauge_alone(cuda, setup):
    net, indeg, gauges, index, store, rows = setup
    hourly, daily = linear_baseline(index, gauges, store, rows, (5, T), tau=TAU, skip_headwaters=False,
                                    max_block_reaches=64, target_blocks=1 << 20)
    assert hourly.shape == (8, T) and daily.shape == (8, 3) and hourly.dtype == torch.float32
    assert bool(torch.isfinite(hourly).all())
    for g, reach in enumerate(gauges):
        h1, d1 = linear_baseline(index, [reach], store, rows, (5, T), tau=TAU, skip_headwaters=False)
        assert np.array_equal(h1[0].cpu().numpy().view(np.uint32), hourly[g].cpu().numpy().view(np.uint32)), g
        assert np.array_equal(d1[0].cpu().numpy().view(np.uint32), daily[g].cpu().numpy().view(np.uint32)), g


def test_hourly_rows_are_the_models(cuda, setup):
    net, indeg, gauges, index, store, rows = setup
    hourly, _ = linear_baseline(index, gauges, store, rows, (5, T), skip_headwaters=False)
    q = store.qr.cpu().numpy()
    r = rows.cpu().numpy()
    qext = np.where(r[None, :] >= 0, q[np.maximum(r, 0), 5:5 + T].T, np.float32(0.001)).astype(np.float32)
    topo = LC.Topology.of_coo(net.n, net.rows, net.cols)  # the tree is its outlet's closure: the union is all of it
    ref = LC.route(topo, np.float32(0.1042 * 86400.0), np.float32(0.3), 3600.0, 1, qext, dtype=np.float32)
    assert np.array_equal(hourly.cpu().numpy().view(np.uint32), ref["end"][gauges].view(np.uint32))


def test_headwaters_and_pooling(cuda, setup):
    net, indeg, gauges, index, store, rows = setup
    routed, _ = linear_baseline(index, gauges, store, rows, (5, T), tau=TAU, skip_headwaters=False)
    hourly, daily = linear_baseline(index, gauges, store, rows, (5, T), tau=TAU)
    head = indeg[gauges] == 0
    assert head.sum() == 2
    nan_rows = torch.isnan(hourly).all(dim=1).cpu().numpy()
    assert np.array_equal(nan_rows, head) and not bool(torch.isnan(hourly[~torch.from_numpy(head)]).any())
    keep = torch.from_numpy(~head).to(cuda)
    assert torch.equal(hourly[keep], routed[keep])
    # [13 + tau : -11 + tau] pooled to len([13 : -11 + tau]) // 24 days (benchmark.py:787-797)
    D = len(range(T)[13:-11 + TAU]) // 24
    want = torch.nn.functional.interpolate(routed[:, 13 + TAU:-11 + TAU].unsqueeze(1), size=(D,), mode="area").squeeze(1)
    assert torch.equal(daily[keep], want[keep]) and bool(torch.isnan(daily[~keep]).all())
    values, count = metrics_device(daily[keep], want[keep] + 0.5)  # the result goes to the metrics as it is
    assert values.shape == (18, int(keep.sum())) and int(count.item()) == 0


def test_arguments(cuda, setup):
    net, indeg, gauges, index, store, rows = setup
    with pytest.raises(ValueError):
        linear_baseline(index, gauges, store, rows, (5, T), irf_fn="hayami")
    with pytest.raises(ValueError):
        linear_baseline(index, gauges, store, rows, (5, 30))
    host = UpstreamIndex(net.n, net.rows, net.cols)
    with pytest.raises(RuntimeError):
        linear_baseline(host, gauges, store, rows, (5, T))
    out, _ = linear_baseline(index, gauges[:2], store, rows, (5, T), irf_fn="linear_storage", skip_headwaters=False)
    assert bool(torch.isfinite(out).all())
