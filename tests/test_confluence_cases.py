"""Reaches with more than two inflows through the host graph builder (csrc/graph.cpp: ``upc`` / ``xoff`` / ``xlist``
emission, virtual-inflow slots in the lists, the list-length accounting of the packer), and the conditions of
tests/test_gpu_confluences.py: every (network, partition) it routes holds the classes of confluence its row in
``confluence_cases.PAIRS`` names, so a GPU test there cannot silently test nothing.

Runs on CPU (``host_only=True``, as test_graph.py).  Reference targets: SciPy ``tocsr()``, the oracle's network
structure, and the reference's PatternMapper layout recorded in tests/golden/confluence.npz.
"""

import numpy as np
import pytest
import scipy.sparse as sp

import confluence_cases as cc
from conftest import load_golden
from ddr_amd import _lib
from ddr_amd.graph import RiverGraph
from oracle import mc_oracle as O

NETS = ["golden300", "bushy600", "bushy2600", "hub", "mix40", "star3", "star17", "star65", "confetti"]
HARD_CAP = 4096  # csrc/internal.h kDefaultBlockReaches
MAX_LIST = 8191  # csrc/internal.h kMaxConfluenceList
LARGEST_STAR = cc.LARGEST_STAR


def host_graph(net, **kw):
    return RiverGraph(net.n, net.rows, net.cols, host_only=True, **kw)


def test_builders_are_topological_trees_with_the_listed_in_degrees():
    for name in ("bushy300", "bushy600", "bushy1500", "bushy2600"):
        net = cc.network(name)
        assert len(net.rows) == net.n - 1 and np.all(net.cols < net.rows)
        indeg = np.bincount(net.rows, minlength=net.n)
        assert set(np.unique(indeg)) >= {0, 3, 4, 5, 6, 9, 14, 15, 16, 17, 20}, name
        np.testing.assert_array_equal(cc.bushy(net.n, 0).rows, net.rows)  # seeded
    assert int((np.bincount(cc.network("bushy2600").rows) >= 15).sum()) >= 50
    for k in cc.STAR_KS:
        net = cc.star(k)
        assert net.n == k + 1 and np.all(net.rows == k) and np.array_equal(net.cols, np.arange(k))
    mix = cc.mix40()
    indeg = np.bincount(mix.rows, minlength=40)
    assert mix.n == 40 and indeg[cc.MIX40_HUB9] == 9 and indeg[cc.MIX40_HUB20] == 20 and indeg[cc.MIX40_OUTLET] == 5
    assert mix.down[cc.MIX40_LEAF20] == cc.MIX40_HUB20 and indeg[cc.MIX40_LEAF20] == 0
    hub = cc.network("hub")
    assert np.bincount(hub.rows, minlength=hub.n)[-1] == 20 and np.bincount(hub.rows).max() == 20
    conf = cc.network("confetti")
    assert len(conf.basin_sizes) == 5000 and set(np.unique(conf.basin_sizes)) == {1, 2, 3}
    # a wave of 64 consecutive reaches holds far more than four distinct basins (devgraph.hip kAggRounds)
    basin = np.repeat(np.arange(5000), conf.basin_sizes)
    assert min(len(np.unique(basin[s:s + 64])) for s in range(0, conf.n - 64, 64)) > 16


def test_classifier_on_a_hand_partition():
    """mix40 split by hand: block 0 = the 9-star's leaves 0..8, block 1 = its hub, the chain and the 20-star's first
    two leaves, block 2 = the rest."""
    net = cc.mix40()
    block = np.zeros(40, np.int64)
    block[9:17] = 1
    block[17:] = 2
    c = cc.classify(block, net)
    np.testing.assert_array_equal(c.ids, [9, 35, 39])
    np.testing.assert_array_equal(c.indeg, [9, 20, 5])
    np.testing.assert_array_equal(c.n_local, [0, 18, 4])
    np.testing.assert_array_equal(c.n_cut, [9, 2, 1])
    np.testing.assert_array_equal(c.cut_pos[0], np.arange(9))
    np.testing.assert_array_equal(c.cut_pos[1], [0, 1])
    np.testing.assert_array_equal(c.cut_pos[2], [0])  # inflows of 39 in column order: 14, 35, 36, 37, 38
    np.testing.assert_array_equal(c.per_block, [0, 1, 2])
    np.testing.assert_array_equal(c.list_len, [0, 9, 25])
    assert c.classes() == {"all_cut", "mixed", "cut_pos0", "cut_pos1", "cut_pos2plus", "two_in_block", "deg17plus"}


@pytest.mark.parametrize("name,part,gkw,need,kr", cc.PAIRS, ids=[f"{p[0]}-{p[1]}" for p in cc.PAIRS])
def test_gpu_pairs_hold_their_classes_of_confluence(name, part, gkw, need, kr):
    net = cc.network(name)
    g = host_graph(net, **gkw)
    c = cc.classify(g.structure()["block"], net)
    have = c.classes()
    assert need <= have, sorted(need - have)
    assert g.info.max_depth + 2 < cc.T  # steady ticks exist
    if kr is not None:
        assert g.info.reaches_per_thread == kr
    if part == "whole":
        assert g.info.n_blocks == 1 and g.info.n_cut == 0
    else:
        assert g.info.n_blocks > 1 and g.info.n_cut > 0
    if part == "gen4":
        assert g.info.generations > 1


def test_gpu_pairs_cover_every_class_and_every_kr():
    have, krs = set(), set()
    for name, part, gkw, need, kr in cc.PAIRS:
        have |= need
        if part == "whole":
            krs.add(kr)
    assert have == cc.ALL_CLASSES == {"all_local", "mixed", "all_cut", "cut_pos0", "cut_pos1", "cut_pos2plus",
                                      "two_in_block", "deg3", "deg14", "deg15", "deg16", "deg17plus"}
    assert krs == {1, 2, 4}
    for k in cc.STAR_KS:  # the star sweep: one block, every inflow local
        g = host_graph(cc.star(k))
        assert g.info.n_blocks == 1 and g.info.max_depth == 2


@pytest.mark.parametrize("name", NETS)
def test_csr_and_structure(name):
    net = cc.network(name)
    a = sp.coo_matrix((np.ones(len(net.rows), np.float32), (net.rows, net.cols)), shape=(net.n, net.n)).tocsr()
    o = O.Network.from_coo(net.n, net.rows, net.cols)
    for gkw in ({}, cc.CUT64):
        g = host_graph(net, **gkw)
        crow, col = g.csr()
        np.testing.assert_array_equal(crow, a.indptr)
        np.testing.assert_array_equal(col, a.indices)
        s = g.structure()
        np.testing.assert_array_equal(s["down"], o.down)
        np.testing.assert_array_equal(s["dist"], o.dist)
        assert g.info.n_basins == len(net.basin_sizes)
        assert g.info.max_depth == o.dist.max() + 1


@pytest.mark.parametrize("name", ["bushy600", "bushy2600", "hub"])
@pytest.mark.parametrize("cap", [64, 160, 1024])
def test_partition_invariants_on_cut_confluences(name, cap):
    """test_graph.py test_partition_invariants' assertions where confluences straddle blocks."""
    net = cc.network(name)
    g = host_graph(net, max_block_reaches=cap, target_blocks=1 << 20, max_resident=1 << 20)
    blk = g.structure()["block"]
    counts = np.bincount(blk)
    assert counts.max() <= cap
    assert g.info.n_blocks == len(counts) and counts.min() > 0
    assert int(np.sum(blk[net.rows] != blk[net.cols])) == g.info.n_cut
    edges = {(int(a), int(b)) for a, b in zip(blk[net.cols], blk[net.rows]) if a != b}
    assert all(a < b for a, b in edges), "a cut edge runs from a later block to an earlier one"
    assert cc.classify(blk, net).list_len.max() < MAX_LIST
    assert g.save_numel(10) == 2 * net.n * 10 + g.info.save_elems_fixed
    assert g.state_numel(10) * 2 == g.save_numel(10)


def test_pattern_mapper_layout_matches_reference_golden():
    d = load_golden("confluence")
    net = cc.network("golden300")
    np.testing.assert_array_equal(net.rows, d["rows"])
    np.testing.assert_array_equal(net.cols, d["cols"])
    for gkw in ({}, cc.CUT64):
        g = host_graph(net, **gkw)
        crow, col = g.csr()
        np.testing.assert_array_equal(crow, d["crow"])
        np.testing.assert_array_equal(col, d["col"])
        mcrow, mcol, src = g.pattern_mapper_layout()
        np.testing.assert_array_equal(mcrow, d["mcrow"])
        np.testing.assert_array_equal(mcol, d["mcol"])
        np.testing.assert_array_equal(src, d["mapidx"])


def _valid(g, net):
    """A graph the builder returned is one the kernels can run: block sizes within the capacity, each block's
    confluence lists below the packed word's 13-bit offset range, producers before consumers."""
    blk = g.structure()["block"]
    assert np.bincount(blk).max() <= HARD_CAP
    assert cc.classify(blk, net).list_len.max() < MAX_LIST
    assert int(np.sum(blk[net.rows] != blk[net.cols])) == g.info.n_cut
    assert np.all(blk[net.cols] <= blk[net.rows])


def _build_or_code(net, **kw):
    try:
        return host_graph(net, **kw), None
    except _lib.DDRError as e:
        assert isinstance(e, ValueError)
        return None, e


def test_star_envelope():
    """How wide a confluence the builder takes.  A 500-inflow star builds (its leaves spread over many blocks, the
    hub importing them); at the default options the widest is LARGEST_STAR, one more raises DDR_ERR_CAPACITY, as do
    2048 and 9000 inflows.  Whatever builds is valid."""
    g, e = _build_or_code(cc.star(500))
    assert e is None and g.info.n_blocks > 1
    _valid(g, cc.star(500))
    g, e = _build_or_code(cc.star(LARGEST_STAR))
    assert e is None
    _valid(g, cc.star(LARGEST_STAR))
    c = cc.classify(g.structure()["block"], cc.star(LARGEST_STAR))
    assert int(c.n_cut[0]) == g.info.n_cut == 1024
    for k, msg in ((LARGEST_STAR + 1, "too many inter-workgroup edges"), (2048, "too many inter-workgroup edges"),
                   (9000, "workgroup LDS budget exceeded")):
        g, e = _build_or_code(cc.star(k))
        if e is None:  # a builder that learns to take it must still emit a valid graph
            _valid(g, cc.star(k))
        assert e is not None and e.code == _lib.DDR_ERR_CAPACITY and msg in str(e), (k, str(e))
    # one block: the list of a 2048-inflow hub fits (2048 < 8191 entries) and the star is a single workgroup
    g, e = _build_or_code(cc.star(2048), **cc.WHOLE)
    assert e is None and g.info.n_blocks == 1 and g.info.reaches_per_thread == 4
    _valid(g, cc.star(2048))
    # other builder arguments either build a valid graph or raise DDR_ERR_CAPACITY
    for k in (500, 1025, 4097, 9000):
        for gkw in (cc.CUT64, cc.CUT160, cc.WHOLE):
            g, e = _build_or_code(cc.star(k), **gkw)
            if e is None:
                _valid(g, cc.star(k))
            else:
                assert e.code == _lib.DDR_ERR_CAPACITY, (k, gkw, str(e))
